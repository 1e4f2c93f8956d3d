"""The class-sharded CoCoOp fit as it is deployed: two processes, one GPU each, the gathers over RCCL (clip_calibration_amd/parallel.py
``shard_gather``).  Rank 0 and rank 1 must hold the same bits after three steps -- SGD, the dynamic loss scale from above the fp16 overflow
point (one skipped step) and Adam -- and both the bits of the local-gather run at G = 2 that a third, single-GPU child makes: RCCL's
movement changes nothing, and the run is tied to everything tests/test_gpu_cocoopshard.py holds.

Needs two GPUs: the count is read without initialising one, and this process never touches a GPU -- every run is a fresh child under its
own ``timeout``, in the manner of tests/test_gpu_prodashard_ranks.py.  Run as a script, this file is that child:
``test_gpu_cocoopshard_ranks.py MODE RANK WORLD DIR``."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_GPUS = torch.cuda.device_count()          # does not initialise the GPU (tests/conftest.py)
CHILD_LIMIT = 180                           # seconds: start-up, the RCCL communicator and three three-step fits on `tiny3`, with a wide margin
# the dynamic route starts at twice the scale at which the static path of this case overflows fp16 (profiles/blockscaler_parity.txt: 2^15)
ROUTES = {"static": dict(grad_scale=256.0), "dynamic": dict(grad_scale="dynamic", scaler={"init_scale": 2.0 ** 16, "backoff_factor": 2.0 ** -5}),
          "adam": dict(grad_scale=256.0, optimizer="adam")}

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(N_GPUS < 2, reason="two ranks need two GPUs")]


def child(mode: str, rank: int, world: int, out_dir: str) -> None:
    """One rank of the RCCL run (mode "rccl"), or all ``world`` ranks over a LocalGather (mode "local"): three steps of CoCoOp, C = 3 on
    ``tiny3`` (shards of 2 and 1 classes), batch 3, per route; the loss history, the master block, the momentum block or Adam's moments and
    the scaler block go to DIR/MODE_RANK.npz."""
    sys.path[:0] = [ROOT, HERE]
    import datetime

    import cocoopfit_ref as cref
    import coopfit_ref as ref
    from clip_calibration_amd import cocoopfit, coopfit, parallel
    from clip_calibration_amd.model import build_model

    torch.cuda.set_device(0)                # the parent shows every child one device
    m = build_model(dict(ref.state_dict("tiny3")), {"trainer": "CoOp"}).cuda()
    c = cref.make_case("tiny3", 3, 4, 3)
    exchange = None
    if mode == "rccl":                      # rank 0's communicator id travels over gloo, as parallel.EmbeddingExchange carries it
        import torch.distributed as dist    # MASTER_ADDR and MASTER_PORT are the parent's: a TCP store on the loopback interface
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        exchange = parallel.EmbeddingExchange(torch.device("cuda", 0), backend="rccl")
        assert exchange.rccl_ranks == world
        shards = lambda: [coopfit.Shard(world, rank, parallel.shard_gather(exchange))]
    else:
        shards = lambda: (lambda local: [coopfit.Shard(world, r, local) for r in range(world)])(coopfit.LocalGather(world))
    f, y, lr = c["feats"].cuda(), c["labels"].cuda(), torch.tensor([2e-3, 1e-3, 5e-4]).cuda()
    out = {}
    for route, kw in ROUTES.items():
        states = [cocoopfit.CoCoOpFitState(m, c["ids"], c["params"], logit_scale=ref.LOGIT_SCALE, momentum=0.9, weight_decay=5e-4, shard=sh, **kw)
                  for sh in shards()]
        st = states[rank if mode == "local" else 0]
        losses = torch.cat([st.step(f, y, lr[k:k + 1], want_loss=True) for k in range(3)])
        torch.cuda.synchronize()
        out.update({f"{route}_loss": losses.cpu().numpy(), f"{route}_params": st.block.cpu().numpy()})
        if st._adam is None:
            out[f"{route}_buf"] = st.buf.cpu().numpy()
        else:
            out.update({f"{route}_exp_avg": st._adam.exp_avg.cpu().numpy(), f"{route}_exp_avg_sq": st._adam.exp_avg_sq.cpu().numpy()})
        if st.dynamic:
            out[f"{route}_block"] = st._scaler.block.cpu().numpy()
    np.savez(os.path.join(out_dir, f"{mode}_{rank}.npz"), **out)
    if exchange is not None:
        exchange.close()


def run_children(specs, out_dir):
    """Start one child per (mode, rank, world, device), each under its own ``timeout -k 10``; wait for all with a limit of this test's own.
    The first that fails or times out fails the test: the others are ended by their process groups (``parallel.end_session``), nothing
    more is started and nothing is tried again."""
    import socket
    import subprocess
    from clip_calibration_amd.parallel import end_session, rank_env
    procs = []
    with socket.socket() as s:              # a free port for the ranks' rendezvous
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    for mode, rank, world, device in specs:
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
    finally:                                # whatever happened: no rank process, wrapper or not, outlives this call
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
    for route in ROUTES:
        for what in ("loss", "params") + (("exp_avg", "exp_avg_sq") if route == "adam" else ("buf",)) + (("block",) if route == "dynamic" else ()):
            k = f"{route}_{what}"
            assert np.isfinite(local[k]).all()
            assert np.array_equal(rank0[k], rank1[k]), k                         # every rank ends a step with the same bits
            assert np.array_equal(rank0[k], local[k]), k                         # and RCCL's movement changes none of them
    assert not np.array_equal(local["static_params"], local["dynamic_params"]) and not np.array_equal(local["static_params"], local["adam_params"])


if __name__ == "__main__":
    child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
