"""What nrc_renderer_render_path buys over the SetCamera + Render loop it replaces, on a 64-view orbit with 4 frames per view: the default
preset (1920 x 1080, fBm cloud 256^3, 6x64 cache, training on) and the MC renderer at 32 vertices.

  python tools/camera_path_rate.py [--renderer nrc|mc|both] [--views 64] [--frames-per-view 4] [--reps 7]
      (a) RenderPath, (b) the SetCamera + Render loop (the baseline: the only way before the call existed), (c) the same number of
      frames from a static camera.  Every repetition renders the whole orbit and is timed by the wall clock around it, with a device
      synchronisation before and after; the repetitions of (a), (b) and (c) are interleaved so that clock drift hits them alike.  One JSON line per
      measurement: median ms/frame, min, max and the spread (max - min) / median over the repetitions.  The verdict line compares (a)
      with (b): a path slower than the loop by more than the loop's own spread is a regression.
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/camera_path_rate.py --renderer mc --mask-only path|loop --views 64
      only the views' masks change hands (one frame of a small MC renderer per view): the trace's k_tile_mask (loop) or
      k_tile_rects + k_tile_mask_words (path) rows are the mask kernels' GPU time on that orbit, each path in a trace of its own.
      With --mask-size WxH (default 1920x1080) and the default preset's 256^3 cloud.

profiles/camera_path_rate.txt is the record of a run."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nrc_hpm_renderer_amd import api, scene as sc  # noqa: E402

W, H = 1920, 1080


def make(kind, scene, cam, w=W, h=H):
    if kind == "mc":
        return api.McHpmRenderer(w, h, 32, False, cam, scene), None
    cfg = api.AppConfig()
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(w, h, False, cam, cfg, scene, nrc), nrc


def render(ren, kind):
    if kind == "mc":
        ren.Render()
    else:
        ren.Render(None, True)


def run(kind, how, ren, views, fpc):
    if how == "path":
        ren.RenderPath(views, fpc, None, train=kind == "nrc", out=False)
    elif how == "loop":
        for v in views:
            ren.SetCamera(None, v)
            for _ in range(fpc):
                render(ren, kind)
    else:
        for _ in range(len(views) * fpc):
            render(ren, kind)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(kind, how, ms_per_frame):
    med = statistics.median(ms_per_frame)
    d = dict(what="camera_path_rate", renderer=kind, how=how, reps=len(ms_per_frame), median_ms_per_frame=med, min=min(ms_per_frame),
             max=max(ms_per_frame), spread=(max(ms_per_frame) - min(ms_per_frame)) / med)
    print(json.dumps(d), flush=True)
    return d


def rates(kind, args):
    vol = sc.cached_volume("cloud", 256, seed=1337)
    scene = sc.make_scene(vol, scene_id=4)
    views = sc.orbit_cameras(args.views, aspect=W / H)
    frames = args.views * args.frames_per_view
    rens = {how: make(kind, scene, views[0]) for how in ("path", "loop", "static")}
    for how, (ren, _) in rens.items():      # warm-up: allocations, the flight selection, clocks
        run(kind, how, ren, views[:4], args.frames_per_view)
    ms = {how: [] for how in rens}
    for _ in range(args.reps):
        for how, (ren, _) in rens.items():
            ms[how].append(timed(lambda: run(kind, how, ren, views, args.frames_per_view)) / frames)
    res = {how: summary(kind, how, ms[how]) for how in rens}
    a, b, c = (res[h]["median_ms_per_frame"] for h in ("path", "loop", "static"))
    print(json.dumps(dict(what="camera_path_verdict", renderer=kind, path_over_loop=a / b, path_over_static=a / c, loop_spread=res["loop"]["spread"],
                          path_not_slower_than_loop=bool(a <= b * (1.0 + res["loop"]["spread"])))), flush=True)
    for ren, nrc in rens.values():
        ren.Destroy()
        if nrc is not None:
            nrc.Destroy()


def mask_only(args):
    w, h = (int(x) for x in args.mask_size.lower().split("x"))
    vol = sc.cached_volume("cloud", 256, seed=1337)
    views = sc.orbit_cameras(args.views, aspect=w / h)
    ren = api.McHpmRenderer(w, h, 1, False, views[0], sc.make_scene(vol, scene_id=4))
    run("mc", args.mask_only, ren, views, 1)
    torch.cuda.synchronize()
    print(json.dumps(dict(what="mask_only", how=args.mask_only, views=args.views, size=[w, h], mask_words=int(ren.TileMask().size))))
    ren.Destroy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--renderer", choices=["nrc", "mc", "both"], default="both")
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--frames-per-view", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mask-only", choices=["path", "loop"], default=None)
    ap.add_argument("--mask-size", default="%dx%d" % (W, H))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions: the verdict rests on their spread")
    if args.mask_only:
        return mask_only(args)
    for kind in (("nrc", "mc") if args.renderer == "both" else (args.renderer,)):
        rates(kind, args)


if __name__ == "__main__":
    main()
