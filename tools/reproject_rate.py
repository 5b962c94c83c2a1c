"""What reprojection (api.Reproject / RenderPath(accumulated_out=)) costs, on the bench scene (fBm cloud 256^3, scene 4) at 1920 x 1080.

  rocprofv3 --kernel-trace -d <dir> -- python tools/reproject_rate.py --trace [--calls 8]
      two views of a 180-view orbit (2 degrees apart), four frames each, with their view AOVs; then `--calls` Reproject calls that carry
      the first view into the second: the trace holds `--calls` dispatches of k_reproject.
      `--trace-csv <file>` (a second step, no GPU) prints from the trace's *_kernel_trace.csv the median time of the kernel and that time
      as a multiple of the time its mandatory traffic takes at `--copy-tbs` -- per pixel 52 bytes streamed (colour and AOV read, colour
      and count written) plus the history pixel's 36 gathered (colour, AOV, count), about 88 -- the measured float4 copy bandwidth of
      SURVEY.md section 8d.
  python tools/reproject_rate.py [--views 64] [--frames-per-view 4] [--reps 7]
      a 64-view orbit through RenderPath with an AOV target, and with an AOV and a reproject target, training on: every repetition renders
      the whole orbit and is timed by the wall clock around it with a device synchronisation before and after; the two are interleaved on
      one renderer.  One JSON line each (median ms per view, min, max, spread) and the verdict: the reproject target's cost per view over
      the orbit with the AOV target alone, and whether it exceeds the spread.

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
BYTES_PER_PIXEL = 52 + 36


def make(api, scene, cam):
    cfg = api.AppConfig()
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(W, H, True, cam, cfg, scene, nrc), nrc


def trace(args):
    import torch
    from nrc_hpm_renderer_amd import api, scene as sc
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4)
    cams = sc.orbit_cameras(180, aspect=W / H)[:2]
    ren, nrc = make(api, scene, cams[0])
    views = []
    for cam in cams:
        ren.SetCamera(None, cam)
        for _ in range(4):
            ren.Render(None, True)
        views.append((ren.GetImage().contiguous().clone(), ren.ViewAov().clone()))
    first = api.Reproject(None, views[0][0], 4.0, views[0][1], cams[0])
    hist = (first[0], first[1], views[0][1], cams[0])
    out, cnt = torch.empty_like(first[0]), torch.empty_like(first[1])
    for _ in range(args.calls):
        api.Reproject(hist, views[1][0], 4.0, views[1][1], cams[1], out=out, out_count=cnt)
    torch.cuda.synchronize()
    medium = views[1][1][..., 0] > 0
    print(json.dumps(dict(what="reproject_trace", size=[W, H], calls=args.calls, pixels_medium=float(medium.float().mean().item()),
                          medium_with_history=float((cnt[medium] > 4.0).float().mean().item()), finite=bool(torch.isfinite(out).all().item()))))
    ren.Destroy()
    nrc.Destroy()


def trace_csv(path, copy_tbs):
    us = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            if "k_reproject" in name:
                us.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    us = us[1:] if len(us) > 1 else us      # (the first dispatch is the history-free call of the first view)
    floor = W * H * BYTES_PER_PIXEL / (copy_tbs * 1e12) * 1e6
    med = statistics.median(us)
    print(json.dumps(dict(what="reproject_kernel_time", size=[W, H], copy_tbs=copy_tbs, bytes_per_pixel=BYTES_PER_PIXEL, mandatory_us=floor, calls=len(us),
                          median_us=med, min_us=min(us), max_us=max(us), over_mandatory=med / floor)))


def orbit(args):
    import torch
    from nrc_hpm_renderer_amd import api, scene as sc
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions: the verdict rests on their spread")
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4)
    views = sc.orbit_cameras(args.views, aspect=W / H)
    aovs = torch.empty((args.views, H, W, 4), device="cuda")
    accum = torch.empty((args.views, H, W, 4), device="cuda")
    counts = torch.empty((args.views, H, W), device="cuda")
    ren, nrc = make(api, scene, views[0])      # ONE renderer for both (tools/view_aov_rate.py says why)
    hows = ("aov", "reproject")

    def run(how, vs):
        n = len(vs)
        ren.RenderPath(vs, args.frames_per_view, None, train=True, out=False, aov_out=aovs[:n],
                       accumulated_out=accum[:n] if how == "reproject" else None, accumulated_counts=counts[:n] if how == "reproject" else None)

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
        res[how] = dict(what="reproject_orbit", how=how, views=args.views, frames_per_view=args.frames_per_view, reps=len(v), median_ms_per_view=med,
                        min=min(v), max=max(v), spread=(max(v) - min(v)) / med)
        print(json.dumps(res[how]), flush=True)
    a, b = res["reproject"]["median_ms_per_view"], res["aov"]["median_ms_per_view"]
    print(json.dumps(dict(what="reproject_orbit_verdict", cost_ms_per_view_over_aov=a - b, reproject_over_aov=a / b, aov_spread=res["aov"]["spread"],
                          within_spread=bool(a <= b * (1.0 + res["aov"]["spread"])))), flush=True)
    ren.Destroy()
    nrc.Destroy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-csv", default=None)
    ap.add_argument("--copy-tbs", type=float, default=None, help="the copy bandwidth the mandatory traffic is timed at, in TB/s (SURVEY.md section 8d)")
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--frames-per-view", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.trace_csv:
        if args.copy_tbs is None:
            raise SystemExit("--trace-csv needs --copy-tbs (SURVEY.md section 8d)")
        return trace_csv(args.trace_csv, args.copy_tbs)
    return trace(args) if args.trace else orbit(args)


if __name__ == "__main__":
    main()
