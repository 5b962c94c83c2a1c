"""What a brick list buys over a dense volume when a live renderer's medium is replaced (nrc_renderer_set_volume_bricks against
nrc_renderer_set_volume), on three subjects: the fBm cloud at 256^3, the smoke plume at 512^3 and the fixture cloud (126 x 86 x 154).

  python tools/volume_bricks_rate.py --subject cloud256|smoke512|fixture --sizes        (c) device bytes per sequence frame, brick count
  python tools/volume_bricks_rate.py --subject S --host-calls 20                       (b) wall time of the host-source call
  python tools/volume_bricks_rate.py --subject S --frames 200 --mc-frames 40           (d) ms/frame with a swap before every frame
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/volume_bricks_rate.py --subject S --rebuild-only 200 --path dense|bricks
      (a) only the device-source calls of one path on a small MC renderer: the rebuild kernels' GPU time, in a trace of its own
      (k_vol_ingest<VolDense<..>, ..> against k_vol_brick_index + k_vol_ingest<VolBricks<..>, ..>; k_vol_cells / k_vol_rows run in both
      paths, so each path gets a trace of its own)

Prints one JSON line per measurement; profiles/volume_bricks_rate.txt is the record of a run."""
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
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def subject(name):
    if name == "cloud256":
        return sc.cached_volume("cloud", 256, seed=1337)
    if name == "smoke512":
        return sc.cached_volume("smoke", 512, seed=1337)
    return np.load(os.path.join(ROOT, "tests", "golden", "cloud_sixteenth_u8.npz"))["density"]


def pair(vol):
    """two frames of a sequence: the subject and the subject shifted by 7 voxels along x"""
    return [vol, np.ascontiguousarray(np.roll(vol, 7, axis=2))]


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def sizes(name, vol):
    origins, bricks = sc.volume_to_bricks(vol)
    nz, ny, nx = vol.shape
    cells = ((nx + 7) // 8) * ((ny + 7) // 8) * ((nz + 7) // 8)
    print(json.dumps(dict(what="sizes", subject=name, dims=[nx, ny, nz], nonzero_voxel_fraction=float((vol != 0).mean()), cells=cells,
                          bricks=len(origins), dense_bytes=int(vol.size), brick_bytes=int(bricks.nbytes + origins.nbytes),
                          ratio=float((bricks.nbytes + origins.nbytes) / vol.size))))


def small_mc(vol):
    return api.McHpmRenderer(64, 64, 4, False, sc.make_camera(aspect=1.0), sc.make_scene(vol, scene_id=4))


def rebuild_only(name, vol, n, path):
    mc = small_mc(vol)
    if path == "dense":
        src = [torch.from_numpy(v).cuda() for v in pair(vol)]
        call = lambda i: mc.SetVolume(src[i % 2])      # noqa: E731
    else:
        src = [tuple(torch.from_numpy(a).cuda() for a in sc.volume_to_bricks(v)) for v in pair(vol)]
        call = lambda i: mc.SetVolumeBricks(*src[i % 2])      # noqa: E731
    timed(call, 4)
    dt = timed(call, n)
    print(json.dumps(dict(what="rebuild_only", subject=name, path=path, calls=n, wall_us_per_call=dt * 1e6)))
    mc.Destroy()


def host_calls(name, vol, n):
    mc = small_mc(vol)
    dense = pair(vol)
    lists = [sc.volume_to_bricks(v) for v in dense]
    out = dict(what="host_source_call", subject=name, calls=n)
    for rep in range(2):      # (both orders: the second pass shows the spread)
        for path, call in (("dense", lambda i: mc.SetVolume(dense[i % 2])), ("bricks", lambda i: mc.SetVolumeBricks(*lists[i % 2]))):
            timed(call, 2)
            out["%s_ms_pass%d" % (path, rep)] = timed(call, n) * 1e3
    print(json.dumps(out))
    mc.Destroy()


def frame_rates(name, vol, frames, mc_frames):
    dense = [torch.from_numpy(v).cuda() for v in pair(vol)]
    lists = [tuple(torch.from_numpy(a).cuda() for a in sc.volume_to_bricks(v)) for v in pair(vol)]
    scene = sc.make_scene(vol, scene_id=4, env=sc.procedural_sky())
    cam = sc.make_camera(aspect=W / H)
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=14, log2_infer_batch_size=21, scene_id=4, primary_ray_length=1,
                        primary_ray_prob=0.0, train_spp=1, train_ring_buf_size=1.0, seed=1337, train_ray_length=32)
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, True, cam, cfg, scene, nrc)
    randoms = sc.frame_randoms(256, seed=1337)

    def nrc_frame(swap):
        def f(i):
            if swap == "dense":
                ren.SetVolume(dense[i % 2])
            elif swap == "bricks":
                ren.SetVolumeBricks(*lists[i % 2])
            ren.SetFrameRandom(randoms[i % 256])
            ren.Render(None, True)
        return f

    out = dict(what="nrc_default_preset_ms_per_frame", subject=name, frames=frames)
    for rep in range(2):
        for swap in ("static", "dense", "bricks"):
            timed(nrc_frame(swap), 40)
            out["%s_pass%d" % (swap, rep)] = timed(nrc_frame(swap), frames) * 1e3
    print(json.dumps(out))
    ren.Destroy()
    nrc.Destroy()
    mc = api.McHpmRenderer(W, H, 32, True, cam, scene)

    def mc_frame(swap):
        def f(i):
            if swap == "dense":
                mc.SetVolume(dense[i % 2])
            elif swap == "bricks":
                mc.SetVolumeBricks(*lists[i % 2])
            mc.SetFrameRandom(randoms[i % 256])
            mc.Render()
        return f

    out = dict(what="mc_path_length_32_ms_per_frame", subject=name, frames=mc_frames)
    for rep in range(2):
        for swap in ("static", "dense", "bricks"):
            timed(mc_frame(swap), 5)
            out["%s_pass%d" % (swap, rep)] = timed(mc_frame(swap), mc_frames) * 1e3
    print(json.dumps(out))
    mc.Destroy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--subject", choices=["cloud256", "smoke512", "fixture"], default="cloud256")
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--host-calls", type=int, default=0, metavar="N")
    ap.add_argument("--frames", type=int, default=0, help="timed NRC frames per measurement")
    ap.add_argument("--mc-frames", type=int, default=40)
    ap.add_argument("--rebuild-only", type=int, default=0, metavar="N")
    ap.add_argument("--path", choices=["dense", "bricks"], default="bricks")
    args = ap.parse_args()
    vol = subject(args.subject)
    if args.sizes:
        sizes(args.subject, vol)
    if not (args.host_calls or args.frames or args.rebuild_only):
        return
    torch.cuda.set_device(0)
    if args.rebuild_only:
        rebuild_only(args.subject, vol, args.rebuild_only, args.path)
    if args.host_calls:
        host_calls(args.subject, vol, args.host_calls)
    if args.frames:
        frame_rates(args.subject, vol, args.frames, args.mc_frames)


if __name__ == "__main__":
    main()
