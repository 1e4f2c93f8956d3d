"""What the sharded fits share (``shard=`` on ``coopfit``, ``prodafit``, ``cocoopfit``; ``vptfit``, ``maplefit``, ``promptsrcfit``): this
project's form of the reference's ``nn.DataParallel``.  One process per GPU; ``Shard(world, rank, gather)`` says which part a state is.

The protocol, once.  A sharded step is a generator of PHASES (each fit state's ``_shard_phases``): a phase is the device work a rank
enqueues up to and including one all-gather, and there is a ``yield`` behind every gather, because what follows reads every rank's
block.  Under RCCL (``gather = parallel.shard_gather(exchange)``) a process runs its one state's phases straight through, and every rank
steps its own state.  A ``LocalGather`` stands in for the communicator where all ``world`` states live in ONE process on one GPU: it is
how the feature runs and is tested on a single GPU, and the oracle an RCCL run is compared with bit for bit.  There the phases run in
lock step -- phase k of rank 0, 1, .., G - 1, then phase k + 1 --, on torch's current stream, and the post of the last rank completes the
gather.  Who drives: the first state that steps.  Its ``step`` steps every rank's state, and the step of another state is refused, so
that nobody takes G steps by stepping every rank's state as under RCCL.  ``drive`` + ``step_all`` are that sequence for a step -- the
caller's host-side checks and draws stand between the two, so they are the driver's alone --, ``report_all`` for the diagnostic entry
points; ``check`` is what the fits refuse under ``shard``.  DESIGN.md "Sharded fits: shared plumbing".
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import ops


class LocalGather:
    """The gather of ``world`` shard states that live in ONE process on one GPU (module docstring): each rank posts its send and receive
    blocks through its own port, and the post that completes the set fills every rank's receive block with device copies, rank-major --
    what ``clipmi_allgather`` leaves."""

    def __init__(self, world: int):
        if isinstance(world, bool) or int(world) != world or world < 1:
            raise ValueError(f"LocalGather: world={world} must be an integer >= 1")
        self.world = int(world)
        self.states = [None] * self.world      # the shard states, filed by their rank as they are made
        self.driver = None                     # the state whose ``step`` steps them all: the first that steps
        self._posts = {}

    def port(self, rank: int):
        """Rank ``rank``'s ``gather(src, dst, bytes_per_rank, stream)``."""
        def gather(src: torch.Tensor, dst: torch.Tensor, nbytes: int, stream: int) -> None:
            self._posts[rank] = (src, dst)
            if len(self._posts) < self.world:
                return
            posts, self._posts = self._posts, {}
            srcs = [posts[r][0].view(-1).view(torch.uint8)[:nbytes] for r in range(self.world)]
            if stream != ops._stream():     # torch enqueues the copies on its current stream: it must be the one the phases launched on
                raise RuntimeError("LocalGather: the gather was asked for on a stream that is not torch's current stream")
            for r in range(self.world):
                out = posts[r][1].view(-1).view(torch.uint8)
                for s in range(self.world):
                    out[s * nbytes:(s + 1) * nbytes].copy_(srcs[s])
        return gather


class Shard:
    """Which part of a sharded fit a state is: ``world`` ranks, this one's ``rank``, and ``gather(src, dst, bytes_per_rank,
    stream)``, which leaves rank r's ``src`` in ``dst[r * bytes_per_rank : (r + 1) * bytes_per_rank]`` on every rank, in stream order
    (``src``, ``dst``: contiguous device tensors).  ``gather``: ``parallel.shard_gather(exchange)`` for one process per GPU over RCCL,
    or a ``LocalGather`` shared by the ``world`` states of one process."""

    def __init__(self, world: int, rank: int, gather):
        for name, v in (("world", world), ("rank", rank)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Shard: {name}={v!r} must be an integer")
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"Shard: rank={rank} outside world={world}")
        self.world, self.rank = int(world), int(rank)
        self.local = gather if isinstance(gather, LocalGather) else None
        if self.local is not None and self.local.world != self.world:
            raise ValueError(f"Shard: world={world} but the LocalGather was made for {self.local.world}")
        if self.local is None and not callable(gather):
            raise ValueError("Shard: gather must be a LocalGather or a callable gather(src, dst, bytes_per_rank, stream)")
        self.gather = self.local.port(self.rank) if self.local is not None else gather

    def peer(self, rank: int) -> "Shard":
        """Rank ``rank`` of the same local world."""
        return Shard(self.world, rank, self.local)


def shard_classes(n_cls: int, world: int, rank: int, who: str = "") -> Tuple[int, int]:
    """Classes [lo, hi) of ``n_cls`` that ``rank`` of ``world`` owns: contiguous, the first ``n_cls mod world`` ranks one class more.
    ``who``: what stands in front of the refusal of ``C < G`` (``check``'s "name: ")."""
    from .parallel import shard_bounds
    if n_cls < world:
        raise ValueError(f"{who}shard: C={n_cls} classes cannot be split over world={world} ranks (C < G: a rank would own no class)")
    return shard_bounds(n_cls, rank, world)


def check(who: str, shard, family: Optional[str] = None, *, n_cls: Optional[int] = None, n_prompt: Optional[int] = None,
          class_token_position: str = "end", grad_scale=None, one_call: bool = False, val=None, final_model: str = "last_step",
          return_operand_stats: bool = False) -> None:
    """What the sharded fits refuse, each by name, before any device call, in the one order all of them keep; a caller passes the facts
    its entry point has, and what it does not pass is not checked (the optimiser is ``fitloop.check_optimizer``'s to refuse).  Only
    the CoOp family passes a position and a ``grad_scale``; only ProDA deals ``n_prompt`` no-class prompts out.  ``family`` keeps each
    family's wording as it was: "coop" (``coopfit``), "block" (the batch-sharded image-tower fits), None (``prodafit``, ``cocoopfit``)."""
    coop, block = family == "coop", family == "block"
    if not isinstance(shard, Shard):
        raise ValueError(f"{who}: shard must be a coopfit.Shard(world, rank, gather), got {type(shard).__name__}")
    if n_cls is not None:
        shard_classes(n_cls, shard.world, shard.rank, "" if coop else f"{who}: ")
    if n_prompt is not None and n_prompt < shard.world:
        raise ValueError(f"{who}: shard: P={n_prompt} no-class prompts cannot be dealt out to world={shard.world} ranks (P < G: a rank would own none)")
    if class_token_position != "end":
        raise ValueError(f"{who}: shard covers class_token_position='end' only, not {class_token_position!r}")
    if isinstance(grad_scale, str):
        raise ValueError(f"{who}: shard needs a static grad_scale; the dynamic loss scale (grad_scale={grad_scale!r}) is not sharded")
    if one_call:
        raise ValueError(f"{who}: shard has no one-call step (one_call=True); the sharded step is the separate calls"
                         + (" around one all-gather" if block else ""))
    if val is not None or final_model == "best_val":
        raise ValueError(f"{who}: shard has no validation: val={'' if coop else ', val_loader='} and final_model='best_val' are not sharded")
    if return_operand_stats:
        raise ValueError(f"{who}: shard returns no operand statistics (return_operand_stats=True)" + (": they are per rank" if block else ""))


def check_batch(who: str, shard: Shard, B: int) -> int:
    """The images per rank of a batch of ``B`` under ``shard``; a batch that does not split evenly is refused."""
    if B % shard.world:
        raise ValueError(f"{who}: a batch of B={B} images does not split over G={shard.world} ranks (B must be a multiple of G; ragged "
                         "batches are not sharded)")
    return B // shard.world


def check_batches(who: str, shard: Optional[Shard], images_or_loader, batch_size, drop_last: bool) -> None:
    """``check_batch`` of the batches ``fitloop.cut_batches`` will cut from a tensor of images -- the full ones and the short last
    one --, before any device call (a loader's batches meet the check in ``step``)."""
    if shard is None or not isinstance(images_or_loader, torch.Tensor) or int(batch_size) < 1:
        return
    N, bs = images_or_loader.shape[0], int(batch_size)
    for B in ([bs] if N >= bs else []) + ([N % bs] if N % bs and not drop_last else []):
        check_batch(who, shard, B)


def shard_states(make, shard: Optional[Shard]):
    """This rank's state from ``make(shard)``: under a ``LocalGather`` all the world's states are made here, one per rank, and the one
    of ``shard.rank`` is returned (its ``step`` then steps them all); otherwise the one state."""
    if shard is None or shard.local is None:
        return make(shard)
    return [make(shard.peer(r)) for r in range(shard.world)][shard.rank]


def file_state(shard: Shard, state) -> None:
    """A new shard state files itself with its local gather (nothing to do under an RCCL gather)."""
    if shard.local is not None:
        shard.local.states[shard.rank], shard.local.driver = state, None      # a new set of states chooses its driver anew


def world_states(shard: Optional[Shard], state, who: str):
    """The states a call on ``state`` serves: ``state`` alone, or all of a local gather's world."""
    local = None if shard is None else shard.local
    if local is None:
        return [state]
    if any(s is None for s in local.states):
        raise ValueError(f"{who}: the LocalGather holds {sum(s is not None for s in local.states)} of its {local.world} shard states; "
                         "make one state per rank before the first step")
    return local.states


def drive(shard: Shard, state, who: str):
    """The states ``state``'s step steps -- the world's, once all are made -- with ``state`` their driver: under a local gather the first
    state that steps drives, and a step of another state is refused."""
    states, local = world_states(shard, state, who), shard.local
    if local is not None:
        if local.driver is None:
            local.driver = state
        if local.driver is not state:
            raise ValueError(f"{who}: under a LocalGather the step of rank {local.driver.shard.rank}'s state steps every rank; "
                             f"rank {shard.rank}'s state must not be stepped as well")
    return states


def run_phases(gens) -> None:
    """Advance the shard states' phase generators in lock step, rank after rank, until they end (they end together: every rank runs the
    same phases).  One generator under an RCCL gather; all ``world`` under a local one, where a phase's last post completes the gather."""
    live = True
    while live:
        for g in gens:
            if next(g, StopIteration) is StopIteration:
                live = False


def step_all(states, state, phases) -> None:
    """``state``'s sharded step on ``drive``'s ``states``: ``phases(s)``, state ``s``'s phase generator, of each, run in lock step.  The
    caller counts its own step as it does without ``shard``; a driven peer's ``steps`` advances with it here."""
    run_phases([phases(s) for s in states])
    for s in states:
        s.steps += s is not state


def run_all(shard: Shard, state, who: str, phases) -> None:
    """A collective every rank enters that is no step (``CoOpFitState.gathered_context``): nobody drives and no counter moves."""
    run_phases([phases(s) for s in world_states(shard, state, who)])


def report_all(shard: Shard, state, who: str, phases):
    """The diagnostic entry points under ``shard``: this rank's report after the phases ``phases(s, report)`` of the world's states, a
    fresh dict per rank, which a state's phases fill INSTEAD of stepping."""
    states = world_states(shard, state, who)
    reports = [{} for _ in states]
    run_phases([phases(s, r) for s, r in zip(states, reports)])
    return reports[states.index(state)]
