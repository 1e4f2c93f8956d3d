"""What class sharding does to a CoOp training step (clip_calibration_amd.coopfit ``shard=``, csrc/shard_train.hip, DESIGN.md
"Class-sharded CoOp fit").  Measurement only; bench.py does not run it.

ViT-B/16 text geometry with synthetic weights, batch 32 of cached image features, n_ctx 16, C = 100 and C = 1000 classes, the live-row
cut on.  For every world size of --worlds that the box has GPUs for, the ranks run as fresh child processes, one GPU each, the gathers
over RCCL (``parallel.shard_gather``); rank 0 times one step between two device events with a synchronisation behind it: the median,
minimum and maximum of --iters windows after --warmup untimed steps.  World 1 takes the unsharded step of the same model in turn with
the sharded one, in the same run: that is the baseline every other figure of the file is read against.  The two gathers and the three
new kernels are timed alone, on the buffers the last step left, and the stash bytes of a rank are recorded.

Every child runs under its own ``timeout -k 10``; the parent stops at the first child that fails and tries nothing again.

Usage: python tools/shardfit_bench.py [--iters 5] [--warmup 2] [--classes 100 1000] [--worlds 1 2 4 8] [--out profiles/shardfit_bench.json]"""
import argparse
import datetime
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHILD_LIMIT = 300      # seconds: the ViT-B/16 text tower's weights, the communicator and 2 x (warmup + iters) steps at up to 1000 classes
MAX_RANKS = 8


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn, iters, warmup, cb):
    ms = []
    for k in range(warmup + iters):
        a, b = cb.events(2)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return spread(ms)


def child(a):
    from clip_calibration_amd import coopfit, ops, parallel, synthetic as syn
    from clip_calibration_amd.model import build_model
    import coopfit_bench as cb

    rank, world = a.child
    torch.cuda.set_device(0)                # the parent shows every child one device
    if world > 1:                           # rank 0's communicator id travels over gloo, as parallel.EmbeddingExchange carries it
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))   # MASTER_ADDR, MASTER_PORT: the parent's
    exchange = parallel.EmbeddingExchange(torch.device("cuda", 0), backend="rccl")
    gather = parallel.shard_gather(exchange)
    model = build_model(dict(syn.synthetic_state_dict(cb.GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    g = torch.Generator().manual_seed(1)
    E, D = syn.GEOMETRIES[cb.GEOM].embed_dim, syn.GEOMETRIES[cb.GEOM].transformer_width
    feats = torch.randn(cb.BATCH, E, generator=g).cuda()
    lr = torch.full((1,), 0.002, device="cuda")
    results = []
    for C in a.classes:
        labels = torch.randint(0, C, (cb.BATCH,), generator=g).cuda()
        ctx = 0.02 * torch.randn(cb.N_CTX, D, generator=g)
        ids = cb.prompt_ids(C)
        st = coopfit.CoOpFitState(model, ids, ctx, shard=coopfit.Shard(world, rank, gather))
        base = coopfit.CoOpFitState(model, ids, ctx) if world == 1 else None
        ms = {"sharded": [], "baseline": []}
        for k in range(a.warmup + a.iters):     # the two states take their steps in turn: a drift of the machine reaches both alike
            for name, s in (("baseline", base), ("sharded", st)):
                if s is None:
                    continue
                e0, e1 = cb.events(2)
                e0.record()
                s.step(feats, labels, lr)
                e1.record()
                torch.cuda.synchronize()
                if k >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        t, stream = st.tower, ops._stream()
        r = {"classes": C, "world": world, "classes_on_rank_0": t.C, "token_rows_per_prompt": t.L, "stash_bytes_per_rank": t.stash_bytes,
             "step_ms": spread(ms["sharded"])}
        if base is not None:
            r["baseline_step_ms"] = spread(ms["baseline"])
            r["baseline_stash_bytes"] = base.tower.stash_bytes
            r["same_bits_as_baseline"] = bool(torch.equal(st.ctx, base.ctx) and torch.equal(st.buf, base.buf))
        # the pieces alone, on the buffers the last step left (every rank enters the gathers)
        r["gather_text_ms"] = timed(lambda: gather(st._send_text, st._all_text, st._send_text.numel() * 4, stream), a.iters, a.warmup, cb)
        r["gather_partial_ms"] = timed(lambda: gather(st._send_part, st._all_part, st._send_part.numel() * 4, stream), a.iters, a.warmup, cb)
        r["shard_compact_ms"] = timed(lambda: ops.shard_compact(st._all_text, C, st._text), a.iters, a.warmup, cb)
        r["ctx_partial_ms"] = timed(lambda: ops.ctx_partial(t.d_embed, t.C, t.n_ctx, st._send_part[0]), a.iters, a.warmup, cb)
        scratch = st.ctx.clone()
        r["ctx_step_gathered_ms"] = timed(lambda: ops.ctx_step_gathered(st._all_part.view(world, -1), t.n_ctx, t.D, st.grad_scale, scratch, None, lr, True,
                                                                        want_grad=False), a.iters, a.warmup, cb)
        results.append(r)
    if rank == 0:
        with open(os.path.join(a.dir, f"world{world}.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f)
    exchange.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--classes", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--worlds", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import coopfit_bench as cb
    from clip_calibration_amd.parallel import end_session, rank_env
    gpus = torch.cuda.device_count()        # does not initialise a GPU: this process never touches one
    out = {"geometry": cb.GEOM, "batch": cb.BATCH, "n_ctx": cb.N_CTX, "iters": a.iters, "warmup": a.warmup, "gpus_on_the_box": gpus,
           "worlds_asked": a.worlds, "worlds_run": [], "worlds_not_run": [], "steps": []}
    with tempfile.TemporaryDirectory() as tmp:
        for world in a.worlds:
            if world > min(gpus, MAX_RANKS):
                out["worlds_not_run"].append(world)
                continue
            common = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--warmup", str(a.warmup), "--dir", tmp, "--classes"] + \
                     [str(c) for c in a.classes]
            with socket.socket() as s:          # a free loopback port for the ranks' rendezvous
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
            # rank r on the r-th of the GPUs this process may see, in a session of its own: ending a child ends its whole process group,
            # the rank under the `timeout` wrapper included (parallel.end_session)
            procs = [subprocess.Popen(["timeout", "-k", "10", str(CHILD_LIMIT)] + common + ["--child", str(r), str(world)], env=rank_env(r, port), cwd=ROOT,
                                      start_new_session=True) for r in range(world)]
            failed = None
            try:
                for r, p in enumerate(procs):   # the first child that fails ends the run: the others are ended and nothing is tried again
                    try:
                        if p.wait(timeout=CHILD_LIMIT + 30) != 0:
                            failed = f"world {world}: rank {r} ended with status {p.returncode}"
                    except subprocess.TimeoutExpired:
                        failed = f"world {world}: rank {r} did not end within {CHILD_LIMIT + 30} s"
                    if failed is not None:
                        break
            finally:
                for p in procs:
                    end_session(p)
            if failed is not None:
                sys.exit(failed)
            got = json.load(open(os.path.join(tmp, f"world{world}.json")))
            out["device"] = got["device"]
            out["worlds_run"].append(world)
            out["steps"] += got["results"]
            for r in got["results"]:
                print(json.dumps(r), flush=True)
    if out["worlds_not_run"]:
        out["note"] = (f"the box has {gpus} GPU(s): world sizes {out['worlds_not_run']} were not measured; the figures below say nothing about them")
        print(out["note"], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
