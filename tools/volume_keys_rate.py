"""What volume keyframes cost and buy (nrc_renderer_set_volume_keys / _set_volume_time / _render_path_timed), on an MI355X.

  (a) rocprofv3 --kernel-trace --stats -d <dir> -- python tools/volume_keys_rate.py --rebuild-only lerp|dense|bricks --dims 256|512 [--calls 200]
      only the rebuild runs, on a small MC renderer: `lerp` is SetVolumeTime at weights strictly between two keys (k_vol_ingest<VolLerp, ...> +
      k_vol_cells + k_vol_rows), `dense` is SetVolume of a device u8 volume (k_vol_ingest<VolDense<false>, ...> + the same two) -- the
      baseline: one kernel template, two voxel sources.  Each in a trace of its own: the two share k_vol_cells and k_vol_rows.  512 is the 256^3 cloud
      doubled along every axis.  The in-between reads twice the source bytes; the ratio is reported, not bounded.  `bricks` is `lerp` on the
      same two keys held as 8^3 brick lists (SetVolumeKeyBricks: k_vol_ingest<VolLerpBricks, ...> + the same two); its line also carries
      the bricks per key, the share of the cells they fill and the device bytes held against the dense keys'.
  (b) python tools/volume_keys_rate.py [--renderer nrc|mc|both] [--views 64] [--frames-per-view 4] [--keys 8] [--reps 7]
      a 64-view orbit, 4 frames per view, of the default preset (1920 x 1080, 6x64 cache, training on) and of the MC renderer at 32
      vertices, over 8 keys of the 256^3 fBm cloud (key k is the cloud rolled by 6 k voxels along x), view v at time v * 7 / 63:
        timed   RenderPath(..., times=...)
        loop    what it replaces: the in-between made by torch on the device, SetVolume + SetCamera + Render per view
        static  RenderPath without times (the medium stands still)
      Every repetition renders the whole orbit between two device synchronisations; the repetitions of the three are interleaved.  One
      JSON line per measurement: median ms/frame, min, max, spread = (max - min) / median.  The verdict: the timed path must not be
      slower than the loop by more than the loop's own spread; the ratio to the static path is reported, not bounded.

--record FILE appends every line printed to FILE as well (profiles/volume_keys_rate.txt is the record of a run)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nrc_hpm_renderer_amd import api, scene as sc  # noqa: E402

W, H = 1920, 1080
RECORD = None


def emit(**d):
    line = json.dumps(d)
    print(line, flush=True)
    if RECORD:
        with open(RECORD, "a") as f:
            f.write(line + "\n")


def rebuild_only(how, dims, calls):
    base = sc.cached_volume("cloud", 256, seed=1337)
    vol = base if dims == 256 else np.ascontiguousarray(base.repeat(2, 0).repeat(2, 1).repeat(2, 2))
    other = np.ascontiguousarray(np.roll(vol, 7, axis=2))
    mc = api.McHpmRenderer(64, 64, 4, False, sc.make_camera(aspect=1.0), sc.make_scene(vol, scene_id=4))
    dv = [torch.from_numpy(vol).cuda(), torch.from_numpy(other).cuda()]
    extra = {}
    if how == "bricks":
        counts, origins, bricks = sc.volumes_to_key_bricks([vol, other])
        mc.SetVolumeKeyBricks(counts, torch.from_numpy(origins).cuda(), torch.from_numpy(bricks).cuda())
        cells = (dims // 8) ** 3
        extra = dict(bricks_per_key=[int(c) for c in counts], cell_share=float(counts.sum()) / (2 * cells), key_bytes_held=mc.VolumeKeyBytes(),
                     dense_key_bytes=2 * int(vol.size))
    else:
        mc.SetVolumeKeys(torch.stack(dv))
    weights = [(1 + 37 * i) % 255 + 1 for i in range(calls)]      # 1 .. 255: never an end of the interval
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        if how != "dense":
            mc.SetVolumeTime(weights[i] / 256.0)
        else:
            mc.SetVolume(dv[i % 2])
    torch.cuda.synchronize()
    emit(what="rebuild_only", how=how, dims=dims, calls=calls, wall_us_per_call=(time.perf_counter() - t0) / calls * 1e6,
         source_bytes_per_call=512 * int(counts.sum()) + 8 * cells if how == "bricks" else int(vol.size) * (2 if how == "lerp" else 1), **extra)
    mc.Destroy()


def make(kind, scene, cam):
    if kind == "mc":
        return api.McHpmRenderer(W, H, 32, False, cam, scene), None
    cfg = api.AppConfig()
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc), nrc


def render(ren, kind):
    if kind == "mc":
        ren.Render()
    else:
        ren.Render(None, True)


def torch_in_between(dkeys, t):
    """scene.volume_at on the device: what a caller without the keys would have to do per view"""
    i, w = sc.key_of_time(t, dkeys.shape[0])
    if w == 0:
        return dkeys[i]
    return ((dkeys[i].to(torch.int32) * (256 - w) + dkeys[i + 1].to(torch.int32) * w + 128) >> 8).to(torch.uint8)


def run(kind, how, ren, views, times, fpc, dkeys):
    train = kind == "nrc"
    if how == "timed":
        ren.RenderPath(views, fpc, None, train=train, out=False, times=times)
    elif how == "static":
        ren.RenderPath(views, fpc, None, train=train, out=False)
    else:
        for v, t in zip(views, times):
            ren.SetVolume(torch_in_between(dkeys, t))
            ren.SetCamera(None, v)
            for _ in range(fpc):
                render(ren, kind)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rates(kind, args):
    cloud = sc.cached_volume("cloud", 256, seed=1337)
    keys = np.ascontiguousarray(np.stack([np.roll(cloud, 6 * k, axis=2) for k in range(args.keys)]))
    dkeys = torch.from_numpy(keys).cuda()
    scene = sc.make_scene(keys[0], scene_id=4)
    views = sc.orbit_cameras(args.views, aspect=W / H)
    times = [float(np.float32(v * (args.keys - 1) / max(args.views - 1, 1))) for v in range(args.views)]
    frames = args.views * args.frames_per_view
    rens = {how: make(kind, scene, views[0]) for how in ("timed", "loop", "static")}
    rens["timed"][0].SetVolumeKeys(dkeys)
    # the timed path against the loop on the same views and times, once, before anything is timed (faster and different is not faster)
    a = rens["timed"][0].RenderPath(views[:3], 1, sc.frame_randoms(3, seed=5), train=False, times=times[:3]).cpu().numpy()
    for i in range(3):
        rens["loop"][0].SetVolume(torch_in_between(dkeys, times[i]))
        rens["loop"][0].SetCamera(None, views[i])
        rens["loop"][0].SetFrameRandom(sc.frame_randoms(3, seed=5)[i])
        if kind == "mc":
            rens["loop"][0].Render()
        else:
            rens["loop"][0].Render(None, False)
        b = rens["loop"][0].GetImage().cpu().numpy()
        if not np.array_equal(a[i].view(np.uint32), b.view(np.uint32)):
            raise SystemExit("view %d of the timed path differs from the loop's" % i)
    for how, (ren, _) in rens.items():      # warm-up: allocations, the flight selection, clocks
        run(kind, how, ren, views[:4], times[:4], args.frames_per_view, dkeys)
    ms = {how: [] for how in rens}
    for _ in range(args.reps):
        for how, (ren, _) in rens.items():
            ms[how].append(timed(lambda: run(kind, how, ren, views, times, args.frames_per_view, dkeys)) / frames)
    res = {}
    for how in rens:
        med = statistics.median(ms[how])
        res[how] = dict(median=med, spread=(max(ms[how]) - min(ms[how])) / med)
        emit(what="volume_keys_rate", renderer=kind, how=how, views=args.views, frames_per_view=args.frames_per_view, keys=args.keys,
             reps=args.reps, median_ms_per_frame=med, min=min(ms[how]), max=max(ms[how]), spread=res[how]["spread"])
    t, l, s = (res[h]["median"] for h in ("timed", "loop", "static"))
    emit(what="volume_keys_verdict", renderer=kind, timed_over_loop=t / l, timed_over_static=t / s, loop_spread=res["loop"]["spread"],
         timed_not_slower_than_loop=bool(t <= l * (1.0 + res["loop"]["spread"])))
    for ren, nrc in rens.values():
        ren.Destroy()
        if nrc is not None:
            nrc.Destroy()


def main():
    global RECORD
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--renderer", choices=["nrc", "mc", "both"], default="both")
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--frames-per-view", type=int, default=4)
    ap.add_argument("--keys", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rebuild-only", choices=["lerp", "dense", "bricks"], default=None)
    ap.add_argument("--dims", type=int, choices=[256, 512], default=256)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--record", default=None, metavar="FILE")
    args = ap.parse_args()
    RECORD = args.record
    if not torch.cuda.is_available():
        raise SystemExit("volume_keys_rate: no GPU -- nothing is measured without one")
    torch.cuda.set_device(0)
    if args.rebuild_only:
        return rebuild_only(args.rebuild_only, args.dims, args.calls)
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions: the verdict rests on their spread")
    if args.keys < 2:
        raise SystemExit("at least 2 keys")
    for kind in (("nrc", "mc") if args.renderer == "both" else (args.renderer,)):
        rates(kind, args)


if __name__ == "__main__":
    main()
