"""What the denoise filter (NrcHpmRenderer.DenoisedFrame / RenderPath(denoised_out=)) costs, on the bench scene (fBm cloud 256^3, scene 4) at
1920 x 1080.

  rocprofv3 --kernel-trace -d <dir> -- python tools/denoise_rate.py --trace [--passes 6] [--calls 8]
      four frames of one view, then `--calls` DenoisedFrame calls of `--passes` passes each: the trace holds calls x passes dispatches of
      k_denoise_pass in launch order (pass p of a call is dispatch p of its group) and `--calls` of k_denoise_pack.
      `--trace-csv <file>` (a second step, no GPU) prints from the trace's *_kernel_trace.csv the median time of every pass, of the packing
      launch, and each as a multiple of the time its mandatory traffic takes at `--copy-tbs` (40 bytes per pixel and pass: 16 colour read,
      8 guide read, 16 written; the pack 24) -- the measured float4 copy bandwidth of SURVEY.md section 8d.
  python tools/denoise_rate.py [--views 64] [--frames-per-view 4] [--reps 7] [--passes 3]
      a 64-view orbit through RenderPath without a target, with an AOV target, and with an AOV and a denoise target, training on: every
      repetition renders the whole orbit and is timed by the wall clock around it with a device synchronisation before and after; the
      three are interleaved on one renderer.  One JSON line each (median ms per view, min, max, spread) and the verdict: the denoise
      target's cost per view over the orbit with the AOV target alone, and whether it exceeds the spread.

docs/MEASUREMENT_LOG.md holds the record of a run."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080


def make(api, scene, cam):
    cfg = api.AppConfig()
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(W, H, True, cam, cfg, scene, nrc), nrc


def trace(args):
    import torch
    from nrc_hpm_renderer_amd import api, scene as sc
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4)
    cam = sc.orbit_cameras(16, aspect=W / H)[3]
    ren, nrc = make(api, scene, cam)
    for _ in range(4):
        ren.Render(None, True)
    p = sc.denoise_params(passes=args.passes)
    for _ in range(args.calls):
        out = ren.DenoisedFrame(p)
    torch.cuda.synchronize()
    solid = float((ren.ViewAov()[..., 0] > 0).float().mean().item())
    print(json.dumps(dict(what="denoise_trace", size=[W, H], passes=args.passes, calls=args.calls, pixels_filtered=solid,
                          finite=bool(torch.isfinite(out).all().item()))))
    ren.Destroy()
    nrc.Destroy()


def trace_csv(path, passes, copy_tbs):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            if "k_denoise_" in name:
                rows.append(("pack" if "k_denoise_pack" in name else "pass", int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[1])
    per_pass = [[] for _ in range(passes)]
    pack, k = [], 0
    for kind, t0, t1 in rows:
        if kind == "pack":
            pack.append((t1 - t0) * 1e-3)
            k = 0
        else:
            per_pass[k % passes].append((t1 - t0) * 1e-3)
            k += 1
    px = W * H
    floor_pass, floor_pack = px * 40 / (copy_tbs * 1e12) * 1e6, px * 24 / (copy_tbs * 1e12) * 1e6
    res = dict(what="denoise_pass_times", size=[W, H], copy_tbs=copy_tbs, mandatory_us_per_pass=floor_pass, calls=len(pack),
               pack_us=statistics.median(pack), pack_over_mandatory=statistics.median(pack) / floor_pack, passes=[])
    for p, v in enumerate(per_pass):
        med = statistics.median(v)
        res["passes"].append(dict(stride=1 << p, median_us=med, min_us=min(v), max_us=max(v), over_mandatory=med / floor_pass))
    print(json.dumps(res))


def orbit(args):
    import torch
    from nrc_hpm_renderer_amd import api, scene as sc
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions: the verdict rests on their spread")
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4)
    views = sc.orbit_cameras(args.views, aspect=W / H)
    aovs = torch.empty((args.views, H, W, 4), device="cuda")
    denoised = torch.empty((args.views, H, W, 4), device="cuda")
    p = sc.denoise_params(passes=args.passes)
    ren, nrc = make(api, scene, views[0])      # ONE renderer for all three (tools/view_aov_rate.py says why)
    hows = ("plain", "aov", "denoise")

    def run(how, vs):
        ren.RenderPath(vs, args.frames_per_view, None, train=True, out=False, aov_out=aovs[:len(vs)] if how != "plain" else None,
                       denoised_out=denoised[:len(vs)] if how == "denoise" else None, denoise_params=p)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for how in hows:      # warm-up: allocations, the flight selection, clocks
        run(how, views[:4])
    ms = {how: [] for how in hows}
    for _ in range(args.reps):
        for how in hows:
            ms[how].append(timed(lambda: run(how, views)) / args.views)
    res = {}
    for how, v in ms.items():
        med = statistics.median(v)
        res[how] = dict(what="denoise_orbit", how=how, views=args.views, frames_per_view=args.frames_per_view, passes=args.passes, reps=len(v),
                        median_ms_per_view=med, min=min(v), max=max(v), spread=(max(v) - min(v)) / med)
        print(json.dumps(res[how]), flush=True)
    a, b, c = res["denoise"]["median_ms_per_view"], res["aov"]["median_ms_per_view"], res["plain"]["median_ms_per_view"]
    print(json.dumps(dict(what="denoise_orbit_verdict", cost_ms_per_view_over_aov=a - b, cost_ms_per_view_over_plain=a - c, denoise_over_aov=a / b,
                          aov_spread=res["aov"]["spread"], within_spread=bool(a <= b * (1.0 + res["aov"]["spread"])))), flush=True)
    ren.Destroy()
    nrc.Destroy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-csv", default=None)
    ap.add_argument("--copy-tbs", type=float, default=None, help="the copy bandwidth the mandatory traffic is timed at, in TB/s (SURVEY.md section 8d)")
    ap.add_argument("--passes", type=int, default=None)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--frames-per-view", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.passes is None:
        args.passes = 6 if (args.trace or args.trace_csv) else 3
    if args.trace_csv:
        if args.copy_tbs is None:
            raise SystemExit("--trace-csv needs --copy-tbs (SURVEY.md section 8d)")
        return trace_csv(args.trace_csv, args.passes, args.copy_tbs)
    return trace(args) if args.trace else orbit(args)


if __name__ == "__main__":
    main()
