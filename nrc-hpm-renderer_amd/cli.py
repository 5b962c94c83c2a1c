"""Headless counterpart of the reference's main loop (src/main.cu:152-419) for the hot path.

    python -m nrc_hpm_renderer_amd.cli [17 positional AppConfig args] [--frames N] [--vdb FILE [FILE ...] | --volume N] ...

The 17 positional arguments are the reference's (src/AppConfig.cpp:154-182); without any, the reference's own defaults apply
(src/main.cu:428-439: HashGrid position encoding, OneBlob direction encoding, 6x64, 4 train batches of 2^14).  Every frame is `NrcHpmRenderer::Render(queue, true)` (src/main.cu:287); with
--benchmark each frame is also evaluated like `Benchmark()` (src/main.cu:140-150): the NRC image without training from the same
camera against a reference image, one line `frame mse relBias CV` in `output/ <config-name>/log.txt` (the literal space is the
reference's, src/main.cu:240,446).  The reference image is `--reference FILE.exr` or, like Reference::GenRefImages
(src/Reference.cpp:566-606), a blended MC render (PATH_LENGTH 64, --ref-frames frames).

Multi-GPU (new): `--gpus N` starts N ranks (python -m torch.distributed.run; or start the module under that
launcher yourself).  The frame is sharded by interleaved strips of 8 pixel columns, the MLP gradients are all-reduced every training
step, the per-frame metrics are reduced over the ranks (five fp64 sums, nrc_compare_images_sharded) and `--export` writes the WHOLE
frame from rank 0 (nrc_renderer_gather_frame).  Rank 0 owns the log.  NRC_CLI_SHARED_GPU=1 rehearses the ranks on one device (gloo).

Animated media (new): `--vdb` with several files is a sequence.  Every file is densified over the union of their bboxes (one grid),
uploaded once, and the renderer steps through them with NrcHpmRenderer.SetVolume, a new file every `--frames-per-volume` frames (the
cache keeps training across the swaps).  `--benchmark` needs a single volume: there is no reference image of a moving medium.
Camera paths (new): `--orbit N` renders an N-view turntable around the volume (scene.orbit_cameras) with one
NrcHpmRenderer.RenderPath call -- `--frames` frames per view, trained like the per-frame loop's -- instead of the loop below; an
`--export` name with a printf integer conversion (out_%04d.exr) then writes one file per view.
With `--bricks` the sequence is held as brick lists instead: every file's 8^3 leaves are read over the union bbox with its minimum
snapped down to multiples of 8 (io_vdb.read_vdb_bricks; no dense array per file on the host or the device) and the renderer steps
through them with NrcHpmRenderer.SetVolumeBricks.  The run prints the device bytes held per file, dense against bricks.
An animated fly-through (new): `--orbit N --vdb a b c --animate` uploads the files as volume keys (NrcHpmRenderer.SetVolumeKeys; key i
at time i) and renders view v at time v * (n_keys - 1) / max(N - 1, 1) * `--time-scale` -- the medium in between two files is their
linear in-between -- with one RenderPath(..., times=...) call.  A --time-scale below 1 is slow motion; times past the last key stay there.
With `--sparse-keys` the keys are held as brick lists (NrcHpmRenderer.SetVolumeKeyBricks): every file's leaves are read over the aligned
union bbox as for `--bricks`, no dense array is made per file (only the first list is densified, for creation), and the run prints the
dense and brick byte counts held.  `--animate --bricks` stays refused: `--bricks` means stepping with SetVolumeBricks.
Denoise (new): `--denoise [PASSES]` with `--export` writes the frame filtered by the AOV-guided a-trous filter (include/nrc_hpm.h, "Denoise")
instead of the raw one; with `--orbit` and a file per view every view's final frame is filtered with its own AOV inside the one RenderPath call.
Reproject (new): `--reproject [MAX_HISTORY]` with `--orbit` and a file per view (`--export` with a `%d` pattern) writes every view's frame
accumulated over the views before it by reprojection (include/nrc_hpm.h, "Reproject"); with `--denoise` the accumulated frames are filtered.
"""
import argparse
import math
import os
import re
import sys

import numpy as np

def export_paths(pattern, n_views):
    """--export: the files a run writes -- a name with a printf integer conversion (out_%04d.exr) once per view, any other name once"""
    if pattern is None:
        return []
    if "%" not in pattern:
        return [pattern]
    if pattern.count("%") != 1 or len(re.findall(r"%0?[0-9]*[di]", pattern)) != 1:
        raise SystemExit("SkyRenderer ERROR: --export %r is not a file name with one integer conversion such as out_%%04d.exr" % pattern)
    return [pattern % k for k in range(n_views)]


def check_orbit_args(args):
    """what --orbit can be combined with (raises SystemExit); returns the number of views, 0 without --orbit"""
    if args.orbit is None:      # (an --export name is then taken literally, as it always was)
        return 0
    if args.orbit < 1:
        raise SystemExit("SkyRenderer ERROR: --orbit must be at least 1")
    if args.frames < 1:
        raise SystemExit("SkyRenderer ERROR: --orbit needs --frames of at least 1 (frames per view)")
    if args.benchmark:
        raise SystemExit("SkyRenderer ERROR: --orbit and --benchmark exclude each other (the reference image belongs to one camera)")
    if args.vdb and len(args.vdb) > 1 and not getattr(args, "animate", False):
        raise SystemExit("SkyRenderer ERROR: --orbit takes one volume, not a --vdb sequence")
    if args.gpus > 1 and args.export and "%" in args.export:
        raise SystemExit("SkyRenderer ERROR: one file per view (--export with %) is not available with --gpus")
    export_paths(args.export, args.orbit)
    return args.orbit


def check_aov_args(args):
    """what --aov can be combined with (raises SystemExit)"""
    if not getattr(args, "aov", False):
        return
    if not args.export:
        raise SystemExit("SkyRenderer ERROR: --aov adds channels to the files --export writes: give --export")
    if args.gpus > 1:
        raise SystemExit("SkyRenderer ERROR: --aov is not available with --gpus (a sharded renderer holds its own columns' AOV only)")


def check_denoise_args(args):
    """what --denoise can be combined with (raises SystemExit)"""
    passes = getattr(args, "denoise", None)
    if passes is None:
        return
    if not 1 <= passes <= 6:
        raise SystemExit("SkyRenderer ERROR: --denoise takes 1 .. 6 passes")
    if not args.export:
        raise SystemExit("SkyRenderer ERROR: --denoise filters the image --export writes: give --export")
    if args.gpus > 1:
        raise SystemExit("SkyRenderer ERROR: --denoise is not available with --gpus (a sharded renderer's local image has no pixel neighbours)")
    if getattr(args, "holdout_sphere", None) is not None:
        raise SystemExit("SkyRenderer ERROR: --denoise and --holdout-sphere exclude each other (the filter's guide is the whole rays' AOV)")


def check_reproject_args(args):
    """what --reproject can be combined with (raises SystemExit)"""
    cap = getattr(args, "reproject", None)
    if cap is None:
        return
    if not 0.0 < cap < math.inf:      # (NaN included)
        raise SystemExit("SkyRenderer ERROR: --reproject takes a MAX_HISTORY > 0")
    if getattr(args, "orbit", None) is None:
        raise SystemExit("SkyRenderer ERROR: --reproject carries frames from view to view: give --orbit")
    if not args.export or "%" not in args.export:
        raise SystemExit("SkyRenderer ERROR: --reproject writes every view's accumulated frame: give --export with a %d pattern")
    if args.gpus > 1:
        raise SystemExit("SkyRenderer ERROR: --reproject is not available with --gpus (a sharded renderer's local image has no pixel neighbours)")
    if getattr(args, "holdout_sphere", None) is not None:
        raise SystemExit("SkyRenderer ERROR: --reproject and --holdout-sphere exclude each other (the guides are the whole rays' AOVs)")


def aov_planes(rgba, aov):
    """the channels of an --aov file from a view's [h][w][4] framebuffer and AOV: what ExportImageWithAovToFile writes"""
    return {"R": rgba[..., 0], "G": rgba[..., 1], "B": rgba[..., 2], "A": aov[..., 0], "tau": aov[..., 1], "Z": aov[..., 2], "Zhalf": aov[..., 3]}


def check_ray_aov_args(args):
    """what --shadow-map and --holdout-sphere can be combined with (raises SystemExit)"""
    radius = getattr(args, "holdout_sphere", None)
    if radius is not None:
        if not getattr(args, "aov", False):
            raise SystemExit("SkyRenderer ERROR: --holdout-sphere holds the --aov export out: give --aov (and --export)")
        if not (math.isfinite(radius) and radius > 0.0):
            raise SystemExit("SkyRenderer ERROR: --holdout-sphere must be a finite radius above 0")
    path = getattr(args, "shadow_map", None)
    if path is not None:
        if not path:
            raise SystemExit("SkyRenderer ERROR: --shadow-map needs a file name")
        if getattr(args, "shadow_size", 1) < 1:
            raise SystemExit("SkyRenderer ERROR: --shadow-size must be at least 1")


DEEP_TAU_MAX = 3.0      # --deep: the levels run up to optical depth 3 (opacity 0.95) in equal steps of opacity


def check_deep_args(args):
    """what --deep can be combined with (raises SystemExit)"""
    k = getattr(args, "deep", None)
    if k is None:
        return
    if not 1 <= k <= 32:
        raise SystemExit("SkyRenderer ERROR: --deep takes 1 .. 32 levels")
    if not getattr(args, "aov", False) and not getattr(args, "shadow_map", None):
        raise SystemExit("SkyRenderer ERROR: --deep adds channels to the --aov export or to the --shadow-map: give one of them")
    if getattr(args, "aov", False) and "%" in (getattr(args, "export", None) or ""):
        raise SystemExit("SkyRenderer ERROR: --deep is not available for a file per view (a path has no deep target)")


def deep_planes(z):
    """the channels Zd00 .. of a --deep export from the planes [K][h][w] (api.DeepViewAov / DeepOrthoAov)"""
    return {"Zd%02d" % k: z[k] for k in range(z.shape[0])}


def write_deep_sidecar(path, levels):
    """the levels of a --deep export beside it: <file without .exr>.json = {"tau_max", "levels", "channels"}; returns the name"""
    import json
    name = os.path.splitext(path)[0] + ".json"
    with open(name, "w") as f:
        json.dump({"tau_max": DEEP_TAU_MAX, "levels": [float(x) for x in levels], "channels": ["Zd%02d" % k for k in range(len(levels))]}, f)
    return name


def shadow_planes(aov):
    """the channels of a --shadow-map file from the light view's [h][w][4] ray AOV"""
    return {"A": aov[..., 0], "tau": aov[..., 1], "Z": aov[..., 2], "Zhalf": aov[..., 3]}


def sphere_depth(rays, radius):
    """--holdout-sphere: the analytic depth image of a sphere of `radius` at the origin along the records rays [...][8] (api.camera_rays:
    unit directions, so the ray parameter is distance) -- float32 [...], the near root, +inf where the ray passes the sphere or starts inside
    or behind it"""
    r = np.asarray(rays, np.float64)
    o, d = r[..., 0:3], r[..., 4:7]
    a, b, c = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - float(radius) ** 2
    disc = b * b - a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(np.where(disc >= 0.0, disc, np.nan))) / a
    return np.where(np.isfinite(t) & (t > 0.0), t, np.inf).astype(np.float32)


def check_animate_args(args):
    """what --animate needs (raises SystemExit); returns whether the run is an animated fly-through"""
    if not getattr(args, "animate", False):
        if getattr(args, "sparse_keys", False):
            raise SystemExit("SkyRenderer ERROR: --sparse-keys goes with --animate (the keys of an animated fly-through held as bricks)")
        return False
    if args.orbit is None or not (args.vdb and len(args.vdb) > 1):
        raise SystemExit("SkyRenderer ERROR: --animate goes with --orbit and a --vdb sequence (several files: the keys)")
    if getattr(args, "bricks", False):
        raise SystemExit("SkyRenderer ERROR: --animate and --bricks exclude each other (--bricks steps a sequence with SetVolumeBricks; --sparse-keys holds "
                         "the keys of --animate as bricks)")
    scale = getattr(args, "time_scale", 1.0)
    if not (math.isfinite(scale) and scale >= 0.0):
        raise SystemExit("SkyRenderer ERROR: --time-scale must be a finite number, at least 0")
    return True


def animate_times(n_views, n_keys, time_scale=1.0):
    """--animate: the time of every view into n_keys keys -- view v at v * (n_keys - 1) / max(n_views - 1, 1) * time_scale, clamped at the
    last key (float32, what RenderPath takes)"""
    last = float(n_keys - 1)
    return np.array([min(v * last / max(n_views - 1, 1) * time_scale, last) for v in range(n_views)], np.float32)


DEFAULT_ARGV = ["RelativeL2Luminance", "Adam", "0.01", "0.99", "0", "0", "64", "6", "21", "14", "4", "4", "1.0", "1", "1", "0.0", "32"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config", nargs="*", help="17 positional AppConfig arguments (all or none)")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--vdb", nargs="+", default=None, help="OpenVDB FloatGrid file(s) (Texture3D::FromVDB semantics); several = a sequence")
    ap.add_argument("--frames-per-volume", type=int, default=1, help="frames rendered with each volume of a --vdb sequence")
    ap.add_argument("--bricks", action="store_true",
                    help="hold a --vdb sequence on the device as lists of 8^3 bricks and step it with SetVolumeBricks (include/nrc_hpm.h, "
                         "nrc_renderer_set_volume_bricks)")
    ap.add_argument("--volume", type=int, default=256, help="edge of the procedural fBm cloud when no --vdb is given")
    ap.add_argument("--env", choices=["white", "black", "sky"], default="white")
    ap.add_argument("--benchmark", action="store_true")
    ap.add_argument("--reference", default=None, help="reference EXR (e.g. reference/4/0.exr of the reference repo)")
    ap.add_argument("--ref-frames", type=int, default=256)
    ap.add_argument("--output", default="output")
    ap.add_argument("--export", default=None, help="write the final NRC image to this EXR; with --orbit a pattern such as out_%%04d.exr writes one file per view")
    ap.add_argument("--aov", action="store_true",
                    help="with --export: the files also carry the view AOV (exact opacity and depth per pixel) as FLOAT channels -- A = alpha "
                         "instead of the framebuffer's constant 1, Z = distance to the first non-empty voxel, Zhalf = distance to optical depth "
                         "ln 2, tau = optical depth -- for compositing; one GPU")
    ap.add_argument("--denoise", type=int, nargs="?", const=3, default=None, metavar="PASSES",
                    help="with --export: the exported R, G, B are the frame filtered by the edge-avoiding a-trous filter that the view AOV guides "
                         "(include/nrc_hpm.h, \"Denoise\"; 1 .. 6 passes, default 3).  Biased: for low frame counts and previews.  Combines with "
                         "--aov; one GPU; not with --holdout-sphere")
    ap.add_argument("--reproject", type=float, nargs="?", const=64.0, default=None, metavar="MAX_HISTORY",
                    help="with --orbit and --export with a %%d pattern: the exported frames are accumulated from view to view by reprojection through "
                         "the view AOV's exact depth (include/nrc_hpm.h, \"Reproject\"; MAX_HISTORY caps the frames history counts for, default "
                         "64).  Biased.  With --denoise the accumulated frames are filtered; one GPU; not with --holdout-sphere")
    ap.add_argument("--holdout-sphere", type=float, default=None, metavar="R",
                    help="with --aov: the AOV is held out to a sphere of radius R at the origin -- the medium in FRONT of the sphere, along each "
                         "camera ray up to the sphere's depth (include/nrc_hpm.h, nrc_renderer_view_aov_to_depth); pixels beside the sphere keep "
                         "the whole ray")
    ap.add_argument("--shadow-map", default=None, metavar="PATH",
                    help="write the medium's shadow map to this EXR: FLOAT channels A, Z, Zhalf, tau along the directional light's rays "
                         "(scene.light_view; include/nrc_hpm.h, nrc_renderer_ortho_aov), of the medium the run ends with")
    ap.add_argument("--deep", type=int, default=None, metavar="K",
                    help="with --aov and/or --shadow-map: K (1 .. 32) more FLOAT channels Zd00 .. Zd<K-1>, the depths at which the pixel's ray "
                         "reaches K optical depths equally spaced in opacity up to tau 3 (scene.deep_levels; include/nrc_hpm.h, \"Deep AOV\"); "
                         "the levels are printed and written beside the file as .json")
    ap.add_argument("--shadow-size", type=int, default=1024, metavar="N", help="--shadow-map: the map is N x N pixels")
    ap.add_argument("--orbit", type=int, default=None, metavar="N",
                    help="render an N-view turntable around the volume with one RenderPath call (include/nrc_hpm.h, nrc_renderer_render_path): "
                         "--frames frames per view")
    ap.add_argument("--animate", action="store_true",
                    help="with --orbit and a --vdb sequence: the files are volume keys and the medium moves through them along the turntable "
                         "(include/nrc_hpm.h, nrc_renderer_render_path_timed)")
    ap.add_argument("--sparse-keys", action="store_true",
                    help="--animate: hold the keys on the device as lists of 8^3 bricks (include/nrc_hpm.h, nrc_renderer_set_volume_key_bricks)")
    ap.add_argument("--time-scale", type=float, default=1.0, help="--animate: the medium's speed (below 1: slow motion; times stop at the last key)")
    ap.add_argument("--orbit-radius", type=float, default=64.0)
    ap.add_argument("--orbit-height", type=float, default=0.0)
    ap.add_argument("--gpus", type=int, default=1, help="ranks the frame is sharded over (one GPU each)")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="training guard: a step whose loss or gradient is not finite is skipped and counted instead of ending the run "
                         "(include/nrc_hpm.h, nrc_cache_set_nonfinite_policy)")
    ap.add_argument("--self-train", action="store_true",
                    help="self-training: train paths end with the cache's own estimate (include/nrc_hpm.h, nrc_config.self_train)")
    args = ap.parse_args(argv)
    if args.benchmark and args.vdb and len(args.vdb) > 1:
        raise SystemExit("SkyRenderer ERROR: --benchmark needs a single --vdb volume (there is no reference image of a moving medium)")
    if args.bricks and not (args.vdb and len(args.vdb) > 1):
        raise SystemExit("SkyRenderer ERROR: --bricks goes with a --vdb sequence (several files)")
    if args.frames_per_volume < 1:
        raise SystemExit("SkyRenderer ERROR: --frames-per-volume must be at least 1")
    animate = check_animate_args(args)
    n_views = check_orbit_args(args)
    check_aov_args(args)
    check_denoise_args(args)
    check_reproject_args(args)
    check_ray_aov_args(args)
    check_deep_args(args)

    if args.gpus > 1 and "RANK" not in os.environ:
        # start the ranks before anything touches the GPU in this process (a process that has initialised HIP must not spawn them)
        import socket
        import subprocess
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), "-m", "nrc_hpm_renderer_amd.cli"] + list(sys.argv[1:] if argv is None else argv)
        return subprocess.call(cmd, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    import torch
    from . import api, io_exr, io_vdb, parallel, scene as sc

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(args.gpus, 1) and "RANK" in os.environ:
        raise SystemExit("SkyRenderer ERROR: --gpus %d but WORLD_SIZE %d" % (args.gpus, world))
    shared_gpu = os.environ.get("NRC_CLI_SHARED_GPU") == "1"

    if args.config and len(args.config) != 17:
        raise SystemExit("SkyRenderer ERROR: Argument count does not match requirements for AppConfig")
    cfg = api.AppConfig(["NRC-HPM-Renderer"] + (args.config or DEFAULT_ARGV))
    if args.self_train:
        cfg.c.self_train = 1
    sequence, brick_lists = [], []
    sparse_keys = animate and args.sparse_keys
    if args.vdb and (args.bricks or sparse_keys):
        # bricks: only the creation volume (the densified first file) exists as a dense array
        bbox = io_vdb.aligned_bbox(io_vdb.union_bbox(args.vdb))
        dims = tuple(int(hi - lo + 1) for lo, hi in zip(bbox[0], bbox[1]))[::-1]      # (nz, ny, nx)
        brick_lists = [io_vdb.read_vdb_bricks(p, bbox) for p in args.vdb]
        for p, (_, b) in zip(args.vdb, brick_lists):
            if len(b) and float(b.max()) != 1.0:      # (Texture3D::FromVDB's check, src/Texture3D.cpp:74)
                raise RuntimeError("SkyRenderer ERROR: VDB is not normalized")
        # (the first list densified: float32 [nz][ny][nx], quantised as quantize_density does)
        density = (sc.bricks_to_volume(*brick_lists[0], dims) * np.float32(255.0)).astype(np.uint8)
    elif args.vdb:
        bbox = io_vdb.union_bbox(args.vdb) if len(args.vdb) > 1 else None
        sequence = [sc.quantize_density(io_vdb.from_vdb(p, bbox)[0]) for p in args.vdb]
        density = sequence[0]
    else:
        density = sc.quantize_density(sc.fbm_cloud_volume(args.volume, seed=1337))
    env = {"white": None, "black": sc.black_env(), "sky": sc.procedural_sky()}[args.env]
    scene = sc.make_scene(density, scene_id=cfg.scene_id, env=env)
    W, H = args.width, args.height
    camera = sc.make_camera(aspect=W / H)            # src/main.cu:180-187
    torch.cuda.set_device(0 if shared_gpu else int(os.environ.get("LOCAL_RANK", "0")))
    tile, lw, cols = None, W, None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if shared_gpu else "nccl", rank=rank, world_size=world)
        tile, lw = parallel.column_tile(rank, world, W, H), parallel.local_width(rank, world, W)
        cols = torch.from_numpy(parallel.rank_columns(rank, world, W)).cuda()
        if (lw * H) % 16:
            raise SystemExit("SkyRenderer ERROR: rank %d's %d x %d tile is not a multiple of 16 pixels" % (rank, lw, H))

    nrc = api.NeuralRadianceCache(cfg)
    if args.skip_nonfinite:
        nrc.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)      # (every rank: the verdicts are identical by construction, no agreement needed)
    if world > 1:
        # one exchange step per train batch: the library's own RCCL all-reduce (one device per rank), or the gloo hook of a rehearsal
        parallel.attach_gradient_allreduce(nrc, world, native=not shared_gpu)
        if shared_gpu:
            nrc.SetCollectiveHooks(rank, world)      # (with the native communicator the gather / metric reduction use RCCL too)
    nrc_renderer = api.NrcHpmRenderer(lw, H, False, camera, cfg, scene, nrc, tile=tile)
    # a sequence: every volume uploaded once, swapped in on the device (every rank swaps the whole volume before the same frame)
    seq_dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in sequence] if len(sequence) > 1 and not animate else []
    # --bricks: every file's list uploaded once (float32 bricks, quantised by the rebuild as the dense path quantises on the host)
    seq_bricks = [(torch.from_numpy(o).cuda(), torch.from_numpy(b).cuda()) for o, b in brick_lists] if not sparse_keys else []
    if seq_bricks and rank == 0:
        for p, (o, b) in zip(args.vdb, seq_bricks):
            held = o.numel() * 4 + b.numel() * 4
            print("%s: %d bricks, %d bytes on the device as float32 bricks (%d as uint8 bricks); dense %d bytes" %
                  (os.path.basename(p), o.shape[0], held, o.numel() * 4 + b.numel(), density.size))
    out_dir = os.path.join(args.output, " " + cfg.GetName())
    log = None
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        log = open(os.path.join(out_dir, "log.txt"), "w")

    ref = None
    if args.benchmark:
        if args.reference:
            ref = torch.from_numpy(io_exr.read_exr(args.reference)).cuda()
            if ref.shape[0] != H or ref.shape[1] != W:
                raise SystemExit("SkyRenderer ERROR: reference image resolution mismatch")     # src/Reference.cpp:627
            if cols is not None:
                ref = ref[:, cols, :].contiguous()      # this rank's columns
        else:
            mc = api.McHpmRenderer(lw, H, 64, True, camera, scene, tile=tile)      # (every rank blends its own columns)
            for _ in range(args.ref_frames):
                mc.Render()
            ref = mc.GetImage().clone()
            mc.Destroy()
        eval_renderer = api.NrcHpmRenderer(lw, H, False, camera, cfg, scene, nrc, tile=tile)        # Reference::CompareNrc renders with train=false

    # A NaN / Inf loss ends the run (src/main.cu:380-384).  With several ranks the decision is COLLECTIVE: the poll below never blocks, so
    # ranks can see the (all-reduced, identical) bad value at different frames -- a rank that left the loop on its own would enter the
    # collective export while its peers are still inside Render()'s gradient exchange, and the job would hang.  Every rank therefore
    # only NOTES a bad loss, the flag is max-reduced every kStopEvery frames (and at the last one), and all ranks leave at that frame.
    kStopEvery = 8
    bad, failed = False, False
    if n_views:
        # a turntable: every view's frames enqueued by one call that does not wait for the GPU; every rank makes the same call
        views = sc.orbit_cameras(n_views, args.orbit_radius, args.orbit_height, aspect=W / H)
        per_view = args.export is not None and "%" in args.export
        times = None
        if animate:      # the files are the keys (uploaded once, from the host), the views' times run through them
            if sparse_keys:      # (from the host, float32 bricks: quantised once at upload, as the dense path quantises on the host)
                nrc_renderer.SetVolumeKeyBricks([len(o) for o, _ in brick_lists], np.ascontiguousarray(np.concatenate([o for o, _ in brick_lists])),
                                                np.ascontiguousarray(np.concatenate([b for _, b in brick_lists])))
                if rank == 0:
                    print("%d keys, %d bricks: %d bytes on the device as brick keys; dense keys %d bytes" %
                          (len(brick_lists), sum(len(o) for o, _ in brick_lists), nrc_renderer.VolumeKeyBytes(), len(brick_lists) * density.size))
            else:
                nrc_renderer.SetVolumeKeys(np.ascontiguousarray(np.stack(sequence)))
            times = animate_times(n_views, nrc_renderer.VolumeKeyCount(), args.time_scale)
        # (--aov: every view's AOV, of its camera and its in-between medium, lands beside its image; the frames are the same frames)
        # (--denoise: every view's final frame filtered with the view's own AOV, which the path then computes whether or not --aov exports it)
        dn = sc.denoise_params(passes=args.denoise) if per_view and args.denoise is not None else None
        # (--reproject: every view's frame accumulated over the views before it; --denoise then filters the accumulated frames)
        rp = sc.reproject_params(max_history=args.reproject) if per_view and args.reproject is not None else None
        aovs = torch.empty((n_views, H, lw, 4), device="cuda", dtype=torch.float32) if per_view and (args.aov or dn is not None or rp is not None) else None
        accumulated = torch.empty((n_views, H, lw, 4), device="cuda", dtype=torch.float32) if rp is not None else None
        denoised = torch.empty((n_views, H, lw, 4), device="cuda", dtype=torch.float32) if dn is not None else None
        depths = None
        if aovs is not None and args.holdout_sphere is not None:
            depths = torch.from_numpy(np.stack([sphere_depth(api.camera_rays(v, lw, H), args.holdout_sphere) for v in views])).cuda()
        images = nrc_renderer.RenderPath(views, args.frames, train=True, out=None if per_view else False, times=times, aov_out=aovs,
                                         aov_depths=depths, denoised_out=denoised, denoise_params=dn, accumulated_out=accumulated, reproject_params=rp)
        loss = nrc.GetLoss(wait=True)
        failed = (math.isnan(loss) or math.isinf(loss)) and not args.skip_nonfinite      # (the all-reduced loss: the same on every rank)
        if failed:
            print("SkyRenderer ERROR: NRC Loss is %s" % loss, file=sys.stderr)
        elif rank == 0:
            print("orbit: %d views x %d frames, loss %.5f" % (n_views, args.frames, loss))
        if per_view and not failed:
            host = (denoised if denoised is not None else accumulated if accumulated is not None else images).cpu().numpy()
            host_aov = aovs.cpu().numpy() if aovs is not None and args.aov else None
            for i, (path, img) in enumerate(zip(export_paths(args.export, n_views), host)):
                if host_aov is not None:
                    io_exr.write_exr_channels(path, aov_planes(img, host_aov[i]))
                else:
                    io_exr.write_exr(path, img)
    for frame in range(0 if n_views else args.frames):
        if seq_dev and frame > 0 and frame % args.frames_per_volume == 0:
            nrc_renderer.SetVolume(seq_dev[(frame // args.frames_per_volume) % len(seq_dev)])
        if seq_bricks and frame > 0 and frame % args.frames_per_volume == 0:
            nrc_renderer.SetVolumeBricks(*seq_bricks[(frame // args.frames_per_volume) % len(seq_bricks)])
        nrc_renderer.Render(None, True)
        loss = nrc.GetLoss(wait=False)          # src/main.cu:376: polled every frame, never blocks the frame pipeline
        if (math.isnan(loss) or math.isinf(loss)) and not args.skip_nonfinite:      # src/main.cu:380-384; with the guard that step was skipped
            print("SkyRenderer ERROR: NRC Loss is %s" % loss, file=sys.stderr)
            bad = True
        if world == 1:
            failed = bad
        elif frame % kStopEvery == kStopEvery - 1 or frame == args.frames - 1:
            flag = torch.tensor([1.0 if bad else 0.0], device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            failed = bool(flag.item() > 0.0)
        if failed:
            break
        if ref is not None:
            eval_renderer.Render(None, False)
            if world > 1:
                r = api.CompareImagesSharded(nrc, ref, eval_renderer.GetImage().contiguous())      # collective: the whole frame's Result
            else:
                r = api.CompareImages(ref, eval_renderer.GetImage())
            rel_bias = (r["own_mean"] - r["ref_mean"]) / r["ref_mean"] if r["ref_mean"] else 0.0
            cv = math.sqrt(max(r["own_var"], 0.0)) / r["own_mean"] if r["own_mean"] else 0.0
            if log is not None:
                log.write("%d %g %g %g\n" % (frame, r["mse"], rel_bias, cv))
        if rank == 0 and (frame % 16 == 0 or frame == args.frames - 1):
            print("frame %d: loss %.5f, %.3f ms" % (frame, loss, nrc_renderer.GetFrameTimeMS()))
    if log is not None:
        log.close()
    if args.skip_nonfinite and rank == 0:
        print("skipped %d of %d steps" % (nrc.GetSkippedSteps()[0], nrc.GetStep()))
    if args.export and not failed and not (n_views and "%" in args.export):
        cam = views[-1] if n_views else camera
        depth = None
        if args.aov and args.holdout_sphere is not None:
            depth = torch.from_numpy(sphere_depth(api.camera_rays(cam, lw, H), args.holdout_sphere)).cuda()
        dn = sc.denoise_params(passes=args.denoise) if args.denoise is not None else None
        colour = (lambda: nrc_renderer.DenoisedFrame(dn)) if dn is not None else nrc_renderer.GetImage
        if args.aov and args.deep:      # the flat AOV and the K depths of one walk (whole rays, or out to the sphere)
            levels = sc.deep_levels(args.deep, DEEP_TAU_MAX)
            z, held = nrc_renderer.DeepViewAov(levels, depth=depth, flat=True)
            planes = aov_planes(colour().cpu().numpy(), held.cpu().numpy())
            planes.update(deep_planes(z.cpu().numpy()))
            io_exr.write_exr_channels(args.export, planes)
            if rank == 0:
                print("deep levels %s -> %s" % (" ".join("%.6g" % x for x in levels), write_deep_sidecar(args.export, levels)))
        elif depth is not None:
            held = nrc_renderer.ViewAovToDepth(depth)
            io_exr.write_exr_channels(args.export, aov_planes(nrc_renderer.GetImage().cpu().numpy(), held.cpu().numpy()))
        elif args.aov and dn is not None:
            nrc_renderer.ExportDenoisedImageToFile(args.export, dn)
        elif args.aov:
            nrc_renderer.ExportImageWithAovToFile(args.export)
        elif dn is not None:
            io_exr.write_exr(args.export, colour().cpu().numpy())
        else:
            nrc_renderer.ExportOutputImageToFile(None, args.export)      # sharded: collective, rank 0 writes the whole frame
    if args.shadow_map and not failed and rank == 0:      # (every rank holds the whole medium: rank 0's map is the map)
        n = args.shadow_size
        if args.deep:      # a deep shadow map: the same four channels and the K depths, one walk
            levels = sc.deep_levels(args.deep, DEEP_TAU_MAX)
            z, shadow = nrc_renderer.DeepOrthoAov(sc.light_view(scene, n, n), n, n, levels, flat=True)
            planes = shadow_planes(shadow.cpu().numpy())
            planes.update(deep_planes(z.cpu().numpy()))
            io_exr.write_exr_channels(args.shadow_map, planes)
            print("deep levels %s -> %s" % (" ".join("%.6g" % x for x in levels), write_deep_sidecar(args.shadow_map, levels)))
        else:
            shadow = nrc_renderer.OrthoAov(sc.light_view(scene, n, n), n, n)
            io_exr.write_exr_channels(args.shadow_map, shadow_planes(shadow.cpu().numpy()))
    nrc_renderer.Destroy()
    if ref is not None:
        eval_renderer.Destroy()
    nrc.Destroy()
    if world > 1:
        if not failed:
            dist.barrier()
        dist.destroy_process_group()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
