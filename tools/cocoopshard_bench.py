"""What class sharding does to a CoCoOp training step (clip_calibration_amd.cocoopfit ``shard=``, csrc/cocoop_train.hip, DESIGN.md
"Class-sharded CoCoOp fit").  Measurement only; bench.py does not run it.

ViT-B/16 text geometry with synthetic weights, batch 1 of cached image features, n_ctx 4, C = 100 and C = 1000 classes, the live-row cut
on.  For every world size of --worlds that the box has GPUs for, the ranks run as fresh child processes, one GPU each, the gathers over
RCCL (``parallel.shard_gather``); rank 0 times one step between two device events with a synchronisation behind it: the median, minimum
and maximum of --iters windows after --warmup untimed steps.  World 1 takes the unsharded step of the same model in turn with the sharded
one, in the same run: that is the baseline the world-1 figure is read against, together with that run's own spread.  The two gathers and
the new kernels are timed alone, on the buffers the last step left, and the stash bytes of rank 0 at G = 1, 2, 4, 8 come from
``cocoopfit.stash_bytes`` whatever was run.

Every child runs under its own ``timeout -k 10``; the parent stops at the first child that fails and tries nothing again.

Usage: python tools/cocoopshard_bench.py [--iters 5] [--warmup 2] [--classes 100 1000] [--worlds 1 2 4 8] [--out profiles/cocoopshard_bench.json]"""
import argparse
import datetime
import json
import os
import socket
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHILD_LIMIT = 420      # seconds: the tower's weights, the communicator and 2 x (warmup + iters) steps of up to 1 000 prompts
MAX_RANKS = 8
STASH_WORLDS = (1, 2, 4, 8)
BATCH = 1


def child(a):
    from clip_calibration_amd import cocoopfit, coopfit, ops, parallel, synthetic as syn
    from clip_calibration_amd.model import build_model
    import cocoopfit_bench as ccb
    import coopfit_bench as cb
    from shardfit_bench import spread, timed

    rank, world = a.child
    torch.cuda.set_device(0)                # the parent shows every child one device
    if world > 1:                           # rank 0's communicator id travels over gloo, as parallel.EmbeddingExchange carries it
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))   # MASTER_ADDR, MASTER_PORT: the parent's
    exchange = parallel.EmbeddingExchange(torch.device("cuda", 0), backend="rccl")
    gather = parallel.shard_gather(exchange)
    model = build_model(dict(syn.synthetic_state_dict(ccb.GEOM, seed=0)), {"trainer": "CoOp"}).cuda()
    g = torch.Generator().manual_seed(1)
    E = syn.GEOMETRIES[ccb.GEOM].embed_dim
    feats = torch.randn(BATCH, E, generator=g).cuda()
    lr = torch.full((1,), 0.002, device="cuda")
    results = []
    for Cn in a.classes:
        labels = torch.randint(0, Cn, (BATCH,), generator=g).cuda()
        ids = ccb.prompt_ids(Cn, ccb.N_CTX)
        params = ccb.params_for(model, feats)
        st = cocoopfit.CoCoOpFitState(model, ids, params, shard=coopfit.Shard(world, rank, gather))
        base = cocoopfit.CoCoOpFitState(model, ids, params) if world == 1 else None
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
        t, stream = st.tower(BATCH), ops._stream()
        r = {"classes": Cn, "world": world, "batch": BATCH, "prompts_on_rank_0": t.N, "prompts": BATCH * Cn, "token_rows_per_prompt": t.L,
             "stash_bytes_per_rank": t.stash_bytes, "text_gather_bytes_per_rank": t.send_text.numel() * 4,
             "partial_gather_bytes_per_rank": t.send_part.numel() * 4, "step_ms": spread(ms["sharded"])}
        if base is not None:
            r["baseline_step_ms"] = spread(ms["baseline"])
            r["baseline_stash_bytes"] = base.tower(BATCH).stash_bytes
            r["same_bits_as_baseline"] = bool(torch.equal(st.block, base.block) and torch.equal(st.buf, base.buf))
        r["stash_bytes_of_rank_0_by_world"] = {str(G): cocoopfit.stash_bytes(model, ids, BATCH, world=G, rank=0)[1] for G in STASH_WORLDS if G <= Cn}
        # the pieces alone, on the buffers the last step left (every rank enters the gathers)
        views = st.params()
        d_text = torch.empty(BATCH * Cn, t.E, dtype=torch.float32, device="cuda").normal_()
        r["gather_text_ms"] = timed(lambda: gather(t.send_text, t.all_text, t.send_text.numel() * 4, stream), a.iters, a.warmup, cb)
        r["gather_partial_ms"] = timed(lambda: gather(t.send_part, t.all_part, t.send_part.numel() * 4, stream), a.iters, a.warmup, cb)
        r["cocoop_embed_classes_ms"] = timed(lambda: ops.cocoop_embed_classes(t.base, views["ctx"], t.meta[2], t.cls_eot, 0, t.n_cls, t.rows, t.prompts, t.eot),
                                             a.iters, a.warmup, cb)
        r["cocoop_shard_compact_ms"] = timed(lambda: ops.cocoop_shard_compact(t.all_text, BATCH, Cn, t.E, t.full_text), a.iters, a.warmup, cb)
        r["cocoop_shard_rows_ms"] = timed(lambda: ops.cocoop_shard_rows(d_text, BATCH, st.lo, st.hi, t.own_d_text), a.iters, a.warmup, cb)
        r["cocoop_dcs_partial_ms"] = timed(lambda: ops.cocoop_dcs_partial(t.d_embed, BATCH, t.n_cls, t.n_ctx, t.send_part), a.iters, a.warmup, cb)
        scratch = torch.empty_like(t.grad)
        r["cocoop_reduce_gathered_ms"] = timed(lambda: ops.cocoop_reduce_gathered(t.all_part, t.meta[0], t.meta[1], views[cocoopfit.NAMES[3]], t.n_ctx,
                                                                                  st.grad_scale, scratch), a.iters, a.warmup, cb)
        results.append(r)
        del st, base
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
    import cocoopfit_bench as ccb
    from clip_calibration_amd.parallel import end_session, rank_env
    gpus = torch.cuda.device_count()        # does not initialise a GPU: this process never touches one
    out = {"geometry": ccb.GEOM, "batch": BATCH, "n_ctx": ccb.N_CTX, "iters": a.iters,
           "warmup": a.warmup, "gpus_on_the_box": gpus, "worlds_asked": a.worlds, "worlds_run": [], "worlds_not_run": [], "steps": []}
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
            # rank r on the r-th of the GPUs this process may see, in a session of its own: ending a child ends its whole process group
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
        out["note"] = (f"the box has {gpus} GPU(s): world sizes {out['worlds_not_run']} were NOT measured; the figures say nothing about them and no "
                       "speed-up is claimed")
        print(out["note"], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
