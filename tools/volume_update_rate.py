"""Frame rate with a new density volume before every frame (nrc_renderer_set_volume), against the static rate of the same renderer in
the same process.  Default preset (bench.py --config c2: 1920x1080, 6x64 fp16 MLP, 16 384 train rays, blended 4-spp steps), four
pre-uploaded 256^3 device volumes (scene.cached_volume("cloud", 256, seed=1337..1340)); then the same pair for McHpmRenderer.

  python tools/volume_update_rate.py [--frames 400] [--mc-frames 60]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/volume_update_rate.py --rebuild-only 200
      (only SetVolume at 256^3 and 512^3 on small MC renderers: the k_vol_* kernels' GPU time, in a trace of their own)

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nrc_hpm_renderer_amd import api, scene as sc  # noqa: E402

W, H, SPP = 1920, 1080, 4


def volumes():
    return [torch.from_numpy(sc.cached_volume("cloud", 256, seed=s)).cuda() for s in range(1337, 1341)]


def timed(frame, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        frame(i)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def nrc_rates(vols, frames, warmup):
    scene = sc.make_scene(vols[0].cpu().numpy(), scene_id=4, env=sc.procedural_sky())
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=14, log2_infer_batch_size=21, scene_id=4, primary_ray_length=1,
                        primary_ray_prob=0.0, train_spp=1, train_ring_buf_size=1.0, seed=1337, train_ray_length=32)
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, True, sc.make_camera(aspect=W / H), cfg, scene, nrc)
    randoms = sc.frame_randoms(SPP * 64, seed=1337)

    def static(i):      # one 4-spp step: blending restarts, four frames enqueued by one call (bench.py's step)
        ren.SetBlend(True)
        ren.RenderFrames(randoms[[(SPP * i + k) % len(randoms) for k in range(SPP)]], True)

    def swapping(i):    # a new volume before every frame (SetVolume restarts blending itself)
        for k in range(SPP):
            ren.SetVolume(vols[(SPP * i + k) % len(vols)])
            ren.SetFrameRandom(randoms[(SPP * i + k) % len(randoms)])
            ren.Render(None, True)

    def static_single(i):      # the same per-frame calls without the swap (Render per frame: no deferred compositing)
        ren.SetBlend(True)
        for k in range(SPP):
            ren.SetFrameRandom(randoms[(SPP * i + k) % len(randoms)])
            ren.Render(None, True)

    out = {}
    steps = frames // SPP
    for name, fn in (("static", static), ("static_per_frame_render", static_single), ("set_volume_every_frame", swapping),
                     ("static_again", static)):
        timed(fn, warmup // SPP)
        dt = timed(fn, steps)
        out[name] = dict(gsamples_s=W * H * SPP * steps / dt / 1e9, ms_per_frame=dt / (steps * SPP) * 1e3)
    # where the time goes: the same pair with one of the renderer's per-view structures switched off (each is rebuilt after a swap)
    for knob, setter in (("cost_order_off", ren.SetCostOrder), ("empty_skip_off", ren.SetEmptySkip), ("hot_tiles_off", ren.SetHotTiles)):
        setter(False)
        pair = {}
        for name, fn in (("static", static_single), ("set_volume_every_frame", swapping)):
            timed(fn, warmup // SPP)
            dt = timed(fn, steps)
            pair[name] = dict(gsamples_s=W * H * SPP * steps / dt / 1e9, ms_per_frame=dt / (steps * SPP) * 1e3)
        setter(True)
        out[knob] = pair
    same = [vols[0]] * len(vols)

    def swapping_same(i):      # SetVolume with the same data every frame: the swap's own cost without new density in the caches
        for k in range(SPP):
            ren.SetVolume(same[k])
            ren.SetFrameRandom(randoms[(SPP * i + k) % len(randoms)])
            ren.Render(None, True)
    timed(swapping_same, warmup // SPP)
    dt = timed(swapping_same, steps)
    out["set_volume_every_frame_same_data"] = dict(gsamples_s=W * H * SPP * steps / dt / 1e9, ms_per_frame=dt / (steps * SPP) * 1e3)
    every = 4

    def swapping_every4(i):    # a new volume every fourth frame (one per 4-spp step)
        for k in range(SPP):
            if (SPP * i + k) % every == 0:
                ren.SetVolume(vols[(SPP * i + k) // every % len(vols)])
            ren.SetFrameRandom(randoms[(SPP * i + k) % len(randoms)])
            ren.Render(None, True)
    timed(swapping_every4, warmup // SPP)
    dt = timed(swapping_every4, steps)
    out["set_volume_every_4th_frame"] = dict(gsamples_s=W * H * SPP * steps / dt / 1e9, ms_per_frame=dt / (steps * SPP) * 1e3)
    losses = []
    for i in range(8):
        swapping(i)
        losses.append(nrc.GetLoss())
    out["ratio_swap_over_static"] = out["set_volume_every_frame"]["gsamples_s"] / max(out["static"]["gsamples_s"], out["static_again"]["gsamples_s"])
    out["loss_trace_while_swapping"] = losses
    ren.Destroy()
    nrc.Destroy()
    return out


def mc_rates(vols, frames):
    scene = sc.make_scene(vols[0].cpu().numpy(), scene_id=4, env=sc.procedural_sky())
    mc = api.McHpmRenderer(W, H, 32, True, sc.make_camera(aspect=W / H), scene)
    randoms = sc.frame_randoms(64, seed=1)

    def static(i):
        mc.SetFrameRandom(randoms[i % 64])
        mc.Render()

    def swapping(i):
        mc.SetVolume(vols[i % len(vols)])
        mc.SetFrameRandom(randoms[i % 64])
        mc.Render()

    out = {}
    for name, fn in (("static", static), ("set_volume_every_frame", swapping), ("static_again", static)):
        timed(fn, 10)
        dt = timed(fn, frames)
        out[name] = dict(gsamples_s=W * H * frames / dt / 1e9, ms_per_frame=dt / frames * 1e3)
    out["ratio_swap_over_static"] = out["set_volume_every_frame"]["gsamples_s"] / max(out["static"]["gsamples_s"], out["static_again"]["gsamples_s"])
    mc.Destroy()
    return out


def rebuild_only(n):
    """SetVolume n times at 256^3 and at 512^3 (the 256^3 cloud doubled along every axis): kernel time comes from the profiler"""
    base = sc.cached_volume("cloud", 256, seed=1337)
    for dims, vol in ((256, base), (512, np.ascontiguousarray(base.repeat(2, 0).repeat(2, 1).repeat(2, 2)))):
        mc = api.McHpmRenderer(64, 64, 4, False, sc.make_camera(aspect=1.0), sc.make_scene(vol, scene_id=4))
        dv = [torch.from_numpy(vol).cuda(), torch.from_numpy(np.ascontiguousarray(np.roll(vol, 7, axis=2))).cuda()]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            mc.SetVolume(dv[i % 2])
        torch.cuda.synchronize()
        print(json.dumps(dict(what="rebuild_only", dims=dims, calls=n, wall_us_per_call=(time.perf_counter() - t0) / n * 1e6)))
        mc.Destroy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=400, help="timed NRC frames per measurement (a multiple of 4)")
    ap.add_argument("--warmup", type=int, default=160)
    ap.add_argument("--mc-frames", type=int, default=60)
    ap.add_argument("--rebuild-only", type=int, default=0, metavar="N")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.rebuild_only:
        rebuild_only(args.rebuild_only)
        return
    vols = volumes()
    print(json.dumps(dict(what="nrc_default_preset", **nrc_rates(vols, args.frames, args.warmup))))
    print(json.dumps(dict(what="mc_path_length_32", **mc_rates(vols, args.mc_frames))))


if __name__ == "__main__":
    main()
