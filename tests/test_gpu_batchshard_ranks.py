"""The batch-sharded MaPLe and VPT fits as they are deployed: two processes, one GPU each, the step's one gather over RCCL
(clip_calibration_amd/parallel.py ``shard_gather``).  Rank 0 and rank 1 must hold the same bits after three steps, and both the bits of
the local-gather run at G = 2 that a third, single-GPU child makes: RCCL's movement changes nothing, and the run is tied to everything
tests/test_gpu_batchshard.py holds.

Needs two GPUs: the count is read without initialising one, and this process never touches a GPU -- every run is a fresh child under its
own ``timeout``.  Run as a script, this file is that child: ``test_gpu_batchshard_ranks.py MODE RANK WORLD DIR``."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_GPUS = torch.cuda.device_count()          # does not initialise the GPU (tests/conftest.py)
FITS = ("maple", "vpt")
CHILD_LIMIT = 180                           # seconds: start-up, the RCCL communicator and two three-step fits on `tiny`, with a wide margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(N_GPUS < 2, reason="two ranks need two GPUs")]


def child(mode: str, rank: int, world: int, out_dir: str) -> None:
    """One rank of the RCCL run (mode "rccl"), or all ``world`` ranks over a LocalGather (mode "local"): three steps of MaPLe (tiny3,
    depth 2) and of VPT (tiny, depth 2) on batches of 4; the loss history, the master block and the momentum buffer go to
    DIR/MODE_RANK.npz."""
    sys.path[:0] = [ROOT, HERE]
    import datetime

    import maplefit_ref
    import vptfit_ref
    from clip_calibration_amd import coopfit, maplefit, parallel, vptfit
    from clip_calibration_amd.model import build_model

    torch.cuda.set_device(0)                # the parent shows every child one device
    exchange = None
    if mode == "rccl":                      # rank 0's communicator id travels over gloo, as parallel.EmbeddingExchange carries it
        import torch.distributed as dist    # MASTER_ADDR and MASTER_PORT are the parent's: a TCP store on the loopback interface
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        exchange = parallel.EmbeddingExchange(torch.device("cuda", 0), backend="rccl")
        assert exchange.rccl_ranks == world
        shards = [coopfit.Shard(world, rank, parallel.shard_gather(exchange))]
    else:
        local = coopfit.LocalGather(world)
        shards = [coopfit.Shard(world, r, local) for r in range(world)]
    sgd = dict(momentum=0.9, weight_decay=5e-4)
    a = maplefit_ref.make_case("tiny3", 2, 1, 5, 4)
    ma = build_model(dict(a["sd"]), maplefit_ref.design(1)).cuda()
    v = vptfit_ref.make_case("tiny", 2, 2, 4, 5)
    mv = build_model(dict(v["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0}).cuda()
    make = {"maple": lambda sh: maplefit.MaPLeFitState(ma, a["ids"], a["pl"], maplefit_ref.LOGIT_SCALE, shard=sh, **sgd),
            "vpt": lambda sh: vptfit.VPTFitState(mv, v["text"].cuda(), vptfit_ref.LOGIT_SCALE, v["prompts"], shard=sh, **sgd)}
    batch = {"maple": (a["images"].cuda(), a["labels"].cuda()), "vpt": (v["images"].cuda(), v["labels"].cuda())}
    lr = torch.tensor([2e-3, 1e-3, 5e-4]).cuda()
    out = {}
    for name in FITS:
        states = [make[name](sh) for sh in shards]
        st = states[rank if mode == "local" else 0]
        x, y = batch[name]
        losses = torch.cat([st.step(x, y, lr[k:k + 1], want_loss=True) for k in range(3)])
        torch.cuda.synchronize()
        out.update({f"{name}_loss": losses.cpu().numpy(), f"{name}_block": st._master().cpu().numpy().reshape(-1), f"{name}_buf": st.buf.cpu().numpy().reshape(-1)})
    np.savez(os.path.join(out_dir, f"{mode}_{rank}.npz"), **out)
    if exchange is not None:
        exchange.close()


def run_children(specs, out_dir):
    """Start one child per (mode, rank, world, device), each under its own ``timeout -k 10``; wait for all with a limit of this test's own.
    The first that fails or times out fails the test: the others are ended -- the rank processes themselves, by their process groups, not
    just their ``timeout`` wrappers (``parallel.end_session``) --, nothing more is started and nothing is tried again."""
    from clip_calibration_amd.parallel import end_session, rank_env
    procs = []
    with socket.socket() as s:              # a free port for the ranks' rendezvous, as tests/test_parallel_gloo.py finds one
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    for mode, rank, world, device in specs:         # the device-th of the GPUs this process may see; a session of its own per child
        log = open(os.path.join(out_dir, f"{mode}_{rank}.log"), "w")
        procs.append((subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), mode, str(rank), str(world),
                                        out_dir], env=rank_env(device, port), cwd=ROOT, stdout=log, stderr=subprocess.STDOUT, start_new_session=True),
                      log, f"{mode}_{rank}"))
    failed = None
    try:
        for p, _, name in procs:
            try:
                if p.wait(timeout=CHILD_LIMIT + 30) != 0:
                    failed = f"{name} ended with status {p.returncode}"
            except subprocess.TimeoutExpired:
                failed = f"{name} did not end within {CHILD_LIMIT + 30} s"
            if failed is not None:
                break
    finally:                                        # whatever happened: no rank process, wrapper or not, outlives this call
        for p, log, _ in procs:
            end_session(p)
            log.close()
    if failed is not None:
        logs = "\n".join(f"--- {name}\n" + open(os.path.join(out_dir, name + ".log")).read()[-2000:] for _, _, name in procs)
        pytest.fail(f"{failed}\n{logs}")
    return [np.load(os.path.join(out_dir, name + ".npz")) for _, _, name in procs]


def test_two_ranks_hold_the_local_gather_bits(tmp_path):
    out_dir = str(tmp_path)
    (local,) = run_children([("local", 0, 2, 0)], out_dir)                       # the oracle: both shard states in one process on one GPU
    rank0, rank1 = run_children([("rccl", 0, 2, 0), ("rccl", 1, 2, 1)], out_dir)
    for name in FITS:
        for what in ("loss", "block", "buf"):
            k = f"{name}_{what}"
            assert np.isfinite(local[k]).all() and local[k].dtype == np.float32
            assert np.array_equal(rank0[k], rank1[k]), k                         # every rank ends a step with the same bits
            assert np.array_equal(rank0[k], local[k]), k                         # and RCCL's movement changes none of them


if __name__ == "__main__":
    child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
