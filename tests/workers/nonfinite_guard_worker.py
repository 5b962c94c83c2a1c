"""Worker of tests/test_gpu_nonfinite_guard.py::test_two_ranks_reach_the_same_verdict: one of TWO ranks, launched by
`python -m torch.distributed.run --nproc-per-node 2`, both on cuda:0, the exchange through the gradient hook and gloo (as
tests/workers/dist_two_rank_worker.py), gradients travelling as fp16 values, NRC_NONFINITE_SKIP on both.  Three training steps on
buffers of the rank's own; in the second, rank 1's targets are 1e5 -- its fp32 gradient is finite but beyond fp16's range -- and rank 0's
are ordinary.  Each rank writes what it saw to <out>.<rank>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    out_path = sys.argv[1]
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nrc_hpm_renderer_amd import api, parallel
    n = 512
    cfg = api.AppConfig(loss_fn="L2", train_batch_count=1, log2_train_batch_size=9)
    nrc = api.NeuralRadianceCache(cfg)
    parallel.attach_gradient_allreduce(nrc, world, native=False, dtype="f16")
    nrc.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
    rng = np.random.default_rng(40 + rank)
    x = torch.empty((n, 5), device="cuda")
    t = torch.empty((n, 3), device="cuda")
    qi, qo = torch.zeros((16, 5), device="cuda"), torch.zeros((16, 3), device="cuda")
    nrc.Init(16, qi, qo, x, t)
    saved = {}
    for step in (1, 2, 3):
        q = rng.random((n, 5), dtype=np.float32)
        q[:, :3] += 31.0
        x.copy_(torch.from_numpy(q))
        y = rng.random((n, 3), dtype=np.float32)
        if step == 2 and rank == 1:
            y[:] = 1.0e5
        t.copy_(torch.from_numpy(y))
        torch.cuda.synchronize()
        if step == 2:
            # this rank's own fp32 gradient of the step, from a cache in the same state that exchanges nothing
            probe = api.NeuralRadianceCache(cfg)
            probe.load_state_dict(nrc.state_dict())
            probe.SetLossNormFactor(world)
            probe.Backward(x, t)
            saved["g_local_bad"] = probe.GetParams(4)[:nrc.ParamCount()]
            probe.Destroy()
            for k, v in zip(("w", "ema", "m", "v"), [nrc.GetParams(i) for i in range(4)]):
                saved[k + "_before_bad"] = v
        nrc.InferAndTrain(None, True)
        torch.cuda.synchronize()
        if step == 2:
            for k, v in zip(("w", "ema", "m", "v"), [nrc.GetParams(i) for i in range(4)]):
                saved[k + "_after_bad"] = v
    state = nrc.state_dict()
    np.savez(out_path + ".%d.npz" % rank, rank=rank, skipped=np.asarray(nrc.GetSkippedSteps(), np.int64), step=state["step"],
             w=state["w"], ema=state["ema"], m=state["m"], v=state["v"], **saved)
    nrc.Destroy()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
