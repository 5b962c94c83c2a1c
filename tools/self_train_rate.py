"""Self-training (include/nrc_hpm.h, nrc_config.self_train): what it costs and what it buys.

rate     the default preset (bench.py --config c2: 1920x1080, 256^3 cloud, 6x64 model, 16 384 train rays and one Adam step per frame,
         blended 4-spp steps through RenderFrames), faithful against self-trained, two renderers in one process, timed in alternating
         blocks after a warm-up long enough for both schedule tuners to settle; plus each one's stage averages (the "train" stage includes
         the tail inference and the combine) and the training stream's busy share from the frame timeline.
quality  relBias / MSE against the reference's EXRs (scenes 0 and 4, 512 training frames, 32 blended evaluation frames: tests/quality.py):
         faithful, Q2 fixed at L = 32, self-trained at L = 1..4 (L > 1 with compat_fix = Q2 and train_ray_length = L).

  python tools/self_train_rate.py [--steps 100] [--blocks 6] [--skip-quality] [--out profiles/self_train_rate.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nrc_hpm_renderer_amd import api, scene as sc  # noqa: E402

W, H, SPP = 1920, 1080, 4


def preset_cfg(self_train):
    return api.AppConfig(train_batch_count=1, log2_train_batch_size=14, log2_infer_batch_size=21, scene_id=4, primary_ray_length=1,
                         primary_ray_prob=0.0, train_spp=1, train_ring_buf_size=1.0, seed=1337, train_ray_length=32, self_train=self_train)


def rate(steps, blocks, warmup_steps, lines):
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4, env=sc.procedural_sky())
    cam = sc.make_camera(aspect=W / H)
    randoms = sc.frame_randoms(SPP * 64, seed=1337)
    runs = {}
    for name, st in (("faithful", 0), ("self_trained", 1)):
        nrc = api.NeuralRadianceCache(preset_cfg(st))
        ren = api.NrcHpmRenderer(W, H, True, cam, preset_cfg(st), scene, nrc)
        runs[name] = dict(nrc=nrc, ren=ren, t=[])

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
        for name in (runs if b % 2 == 0 else list(runs)[::-1]):
            runs[name]["t"].append(step_block(runs[name]["ren"], steps))
    fps = {}
    for name, r in runs.items():
        per_frame = np.array(r["t"]) / (steps * SPP)
        fps[name] = 1.0 / float(np.median(per_frame))
        sched = r["ren"].GetSchedule()
        r["ren"].StageStats(reset=True)
        step_block(r["ren"], 25)
        tl = r["ren"].FrameTimeline(max_frames=SPP * 25)
        st = r["ren"].StageStats(reset=True)
        loss = r["nrc"].GetLoss()
        lines.append("rate %-13s %8.1f frames/s  %7.1f Msamples/s  median %.4f ms/frame (blocks %s)  loss %.5f  schedule %s"
                     % (name, fps[name], fps[name] * W * H / 1e6, 1e3 / fps[name], " ".join("%.4f" % (1e3 * x) for x in per_frame), loss,
                        sched.get("source")))
        lines.append("stages %-11s gen_rays %.4f  prep_train %.4f  infer %.4f  train %.4f  composite %.4f  total %.4f ms (averages over %d frames; "
                     "stages overlap)" % (name, st["gen_rays"], st["prep_train"], st["infer"], st["train"], st["render"], st["total"], st["frames"]))
        if len(tl) > 4:
            span = tl[-1, 5] - tl[0, 0]
            busy = float(np.sum(tl[:, 5] - np.maximum(tl[:, 2], np.concatenate([[tl[0, 2]], tl[:-1, 5]]))))
            lines.append("timeline %-9s %d frames in %.3f ms: %.4f ms/frame; training stream from max(train rays done, previous training done) "
                         "to training done: %.4f ms/frame" % (name, len(tl), span, span / len(tl), busy / len(tl)))
            lines.append("timeline %-9s per frame, ms after its gen_rays start: gen_rays done | train rays done | inference done | "
                         "composite done | training done | next gen_rays start" % name)
            for f in range(len(tl) - 8, len(tl) - 1):
                t0 = tl[f, 0]
                lines.append("  frame %3d  %.4f | %.4f | %.4f | %.4f | %.4f | %.4f" % (f, tl[f, 1] - t0, tl[f, 2] - t0, tl[f, 3] - t0, tl[f, 4] - t0,
                                                                          tl[f, 5] - t0, tl[f + 1, 0] - t0))
    lines.append("rate self_trained / faithful = %.3f (goal, unmeasured before this run: >= 0.90)" % (fps["self_trained"] / fps["faithful"]))
    for r in runs.values():
        r["ren"].Destroy()
        r["nrc"].Destroy()


def quality_table(lines):
    import quality
    cloud = np.load(os.path.join(ROOT, "tests", "golden", "cloud_sixteenth_u8.npz"))["density"]
    cam = sc.make_camera(aspect=quality.W / quality.H)
    lines.append("# quality: scene case | vs EXR relBias mse | loss  (512 training frames, 32 blended evaluation frames, 1920x1080; "
                 "window of the Q2-fixed trainer: relBias %s)" % (quality.bounds(0)["q2_rel_bias"],))
    for sid in (0, 4):
        scene = sc.make_scene(cloud, scene_id=sid)
        refs = dict(exr=quality.load_exr(torch, sid))
        cases = [("faithful", quality.nrc_config(api, sid, False)), ("q2_fixed_L32", quality.nrc_config(api, sid, True))]
        cases += [("self_trained_L%d" % L, quality.nrc_config(api, sid, L > 1, train_ray_length=L if L > 1 else 32, self_train=1))
                  for L in (1, 2, 3, 4)]
        for name, cfg in cases:
            t0 = time.perf_counter()
            r = quality.train_and_evaluate(torch, api, sc, scene, cam, cfg, 512, 32, refs)
            lines.append("scene %d %-16s %+.4f %.5f | %.5f   (%.1f s)" % (sid, name, r["exr"]["rel_bias"], r["exr"]["mse"], r["loss"],
                                                                       time.perf_counter() - t0))
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="4-spp steps per timed block")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=150, help="4-spp steps of warm-up per renderer (the schedule tuner needs ~400 frames)")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/self_train_rate.py, build %s, %s" % (api.build_id(), torch.cuda.get_device_name(0))]
    rate(args.steps, args.blocks, args.warmup, lines)
    print("\n".join(lines), flush=True)
    if not args.skip_quality:
        quality_table(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
