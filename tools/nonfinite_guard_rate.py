"""The training guard (include/nrc_hpm.h, nrc_cache_set_nonfinite_policy): what NRC_NONFINITE_SKIP costs when every step is good.

step     Backward + OptimizerStep alone, 16 384 rays, the 6x64 and the 8x128 model, two caches in one process (guard off / on), timed in
         alternating blocks with HIP events, medians.
preset   the default preset (bench.py --config c2: 1920x1080, 256^3 cloud, 6x64 model, 16 384 train rays and one Adam step per frame, blended
         4-spp steps through RenderFrames), guard off against on, two renderers in one process, alternating blocks after a warm-up long
         enough for both schedule tuners to settle.  The renderer created SECOND in a process runs at 0.55 ms/frame instead of 0.235
         whatever its policy (measured with both orders; not understood, and not the guard's doing), so without --order the preset is run
         in two fresh child processes, once in each order, and the figures compared are those of the renderer created first.

  python tools/nonfinite_guard_rate.py [--steps 100] [--blocks 6] [--skip-preset] [--skip-step] [--order off,on] [--out profiles/nonfinite_guard_rate.txt]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nrc_hpm_renderer_amd import api, scene as sc  # noqa: E402

W, H, SPP = 1920, 1080, 4


def step_rate(lines, blocks, reps):
    n = 16384
    rng = np.random.default_rng(0)
    q = rng.random((n, 5), dtype=np.float32)
    q[:, :3] += 31.0
    x, t = torch.from_numpy(q).cuda(), torch.rand((n, 3), device="cuda")
    for name, kw in (("6x64", dict()), ("8x128", dict(nn_width=128, nn_depth=8))):
        caches = {}
        for policy in ("off", "on"):
            c = api.NeuralRadianceCache(api.AppConfig(**kw))
            if policy == "on":
                c.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
            for _ in range(50):
                c.Backward(x, t)
                c.OptimizerStep()
            caches[policy] = (c, [])
        torch.cuda.synchronize()
        for b in range(blocks):
            for policy in (("off", "on") if b % 2 == 0 else ("on", "off")):
                c, times = caches[policy]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    c.Backward(x, t)
                    c.OptimizerStep()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / reps)
        med = {p: float(np.median(caches[p][1])) for p in caches}
        lines.append("step %-6s guard off %.2f us  on %.2f us  on / off = %.4f   (blocks off: %s | on: %s)  skipped %d" %
                     (name, med["off"], med["on"], med["on"] / med["off"], " ".join("%.2f" % v for v in caches["off"][1]),
                      " ".join("%.2f" % v for v in caches["on"][1]), caches["on"][0].GetSkippedSteps()[0]))
        for c, _ in caches.values():
            c.Destroy()


def preset_cfg():
    return api.AppConfig(train_batch_count=1, log2_train_batch_size=14, log2_infer_batch_size=21, scene_id=4, primary_ray_length=1,
                         primary_ray_prob=0.0, train_spp=1, train_ring_buf_size=1.0, seed=1337, train_ray_length=32)


def preset_rate(lines, steps, blocks, warmup_steps, order):
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4, env=sc.procedural_sky())
    cam = sc.make_camera(aspect=W / H)
    randoms = sc.frame_randoms(SPP * 64, seed=1337)
    runs = {}
    for policy in order:      # (which renderer is created first is part of the experiment: --order)
        nrc = api.NeuralRadianceCache(preset_cfg())
        if policy == "on":
            nrc.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
        runs[policy] = dict(nrc=nrc, ren=api.NrcHpmRenderer(W, H, True, cam, preset_cfg(), scene, nrc), t=[])

    def step_block(ren, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            ren.SetBlend(True)
            ren.RenderFrames(randoms[[(SPP * i + k) % len(randoms) for k in range(SPP)]], True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for r in runs.values():
        step_block(r["ren"], warmup_steps)
    for b in range(blocks):
        for policy in (order if b % 2 == 0 else order[::-1]):
            runs[policy]["t"].append(step_block(runs[policy]["ren"], steps))
    fps = {}
    for policy, r in runs.items():
        per_frame = np.array(r["t"]) / (steps * SPP)
        fps[policy] = 1.0 / float(np.median(per_frame))
        lines.append("preset (created %s) guard %-3s %8.1f frames/s  median %.4f ms/frame (blocks %s)  loss %.5f  skipped %d of %d  schedule %s" %
                     ("first" if policy == order[0] else "second", policy, fps[policy], 1e3 / fps[policy], " ".join("%.4f" % (1e3 * v) for v in per_frame), r["nrc"].GetLoss(),
                      r["nrc"].GetSkippedSteps()[0], r["nrc"].GetStep(), r["ren"].GetSchedule().get("source")))
    if len(fps) == 2:      # (--order on / --order off: one renderer alone in the process)
        lines.append("preset on / off = %.4f frames/s ratio (goal: within the run-to-run spread of the unguarded preset, 1-2 %%)" % (fps["on"] / fps["off"]))
    for r in runs.values():
        r["ren"].Destroy()
        r["nrc"].Destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="4-spp steps per timed block of the preset")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=400, help="training steps per timed block of the step rate")
    ap.add_argument("--warmup", type=int, default=150, help="4-spp steps of warm-up per renderer (the schedule tuner needs ~400 frames)")
    ap.add_argument("--skip-preset", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--order", default=None, help="the order the preset's two renderers are created in, in THIS process (off,on / on,off); "
                                                  "one name: that renderer alone.  Default: both orders, each in a child process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/nonfinite_guard_rate.py, build %s, %s" % (api.build_id(), torch.cuda.get_device_name(0))]
    if not args.skip_step:
        step_rate(lines, args.blocks, args.reps)
    print("\n".join(lines), flush=True)
    n0 = len(lines)
    if not args.skip_preset and args.order:
        preset_rate(lines, args.steps, args.blocks, args.warmup, args.order.split(","))
    elif not args.skip_preset:
        first = {}
        for order in ("off,on", "on,off"):
            with tempfile.NamedTemporaryFile("r", suffix=".txt") as tmp:
                subprocess.run([sys.executable, os.path.abspath(__file__), "--skip-step", "--order", order, "--steps", str(args.steps), "--blocks",
                                str(args.blocks), "--warmup", str(args.warmup), "--out", tmp.name], check=True, timeout=600, stdout=subprocess.DEVNULL)
                for ln in tmp.read().splitlines():
                    if ln.startswith("preset (created"):
                        lines.append("order %s: %s" % (order, ln))
                        m = re.match(r"preset \(created first\) guard (\w+)\s+[\d.]+ frames/s  median ([\d.]+) ms/frame", ln)
                        if m:
                            first[m.group(1)] = float(m.group(2))
        lines.append("preset, each policy as the renderer created first in its process: guard off %.4f ms/frame  on %.4f ms/frame  on / off = %.4f "
                     "(goal: within the run-to-run spread of the unguarded preset, 1-2 %%)" % (first["off"], first["on"], first["on"] / first["off"]))
    print("\n".join(lines[n0:]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
