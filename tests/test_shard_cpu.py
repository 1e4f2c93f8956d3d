"""CPU checks of the sharded fits' shared plumbing (clip_calibration_amd/shard.py): every refusal of ``shard.check`` with the full text
its family has always raised -- the strings below were recorded from ``coopfit._check_shard``, ``prodafit.check_shard``,
``cocoopfit.check_shard``, ``vptfit.check_shard`` and the four gradient entry points before those were folded into ``check`` --, the
order of the refusals where a call breaks two rules, and the driver (``run_phases``, ``world_states``, ``drive``, ``step_all``,
``run_all``, ``report_all``) on plain Python stand-ins for the fit states.  No device, no model."""
import pytest

from clip_calibration_amd import coopfit, shard  # noqa: E402

two = lambda: shard.Shard(2, 0, shard.LocalGather(2))
eight = lambda: shard.Shard(8, 3, shard.LocalGather(8))
VAL = (1, 2)

TYPE = "f: shard must be a coopfit.Shard(world, rank, gather), got tuple"
C_LT_G = "shard: C=5 classes cannot be split over world=8 ranks (C < G: a rank would own no class)"
P_LT_G = "f: shard: P=4 no-class prompts cannot be dealt out to world=8 ranks (P < G: a rank would own none)"
POSITION = "f: shard covers class_token_position='end' only, not 'middle'"
DYNAMIC = "f: shard needs a static grad_scale; the dynamic loss scale (grad_scale='dynamic') is not sharded"
ONE_CALL = "f: shard has no one-call step (one_call=True); the sharded step is the separate calls"
VAL_COOP = "f: shard has no validation: val= and final_model='best_val' are not sharded"
VAL_LONG = "f: shard has no validation: val=, val_loader= and final_model='best_val' are not sharded"
STATS = "f: shard returns no operand statistics (return_operand_stats=True)"

COOP = dict(n_cls=5, class_token_position="end", grad_scale=4096.0)
PRODA = dict(n_cls=5, n_prompt=8)
REFUSALS = [
    # the CoOp family (coopfit): its C < G text carries no name, its validation text no val_loader=
    ("coop", (2, 0), COOP, TYPE),
    ("coop", eight, COOP, C_LT_G),
    ("coop", two, dict(COOP, class_token_position="middle"), POSITION),
    ("coop", two, dict(COOP, grad_scale="dynamic"), DYNAMIC),
    ("coop", two, dict(COOP, val=VAL), VAL_COOP),
    ("coop", two, dict(COOP, final_model="best_val"), VAL_COOP),
    ("coop", two, dict(COOP, return_operand_stats=True), STATS),
    ("coop", two, dict(one_call=True), ONE_CALL),                                             # CoOpFitState.step's, by itself
    ("coop", eight, dict(COOP, class_token_position="middle", grad_scale="dynamic", val=VAL), C_LT_G),       # two rules at once: the order
    ("coop", two, dict(COOP, class_token_position="middle", grad_scale="dynamic", val=VAL), POSITION),
    ("coop", two, dict(COOP, grad_scale="dynamic", val=VAL, return_operand_stats=True), DYNAMIC),
    ("coop", two, dict(COOP, val=VAL, return_operand_stats=True), VAL_COOP),
    # ProDA
    (None, (2, 0), PRODA, TYPE),
    (None, eight, PRODA, "f: " + C_LT_G),
    (None, eight, dict(n_cls=9, n_prompt=4), P_LT_G),
    (None, two, dict(PRODA, one_call=True), ONE_CALL),
    (None, two, dict(PRODA, val=VAL), VAL_LONG),
    (None, two, dict(PRODA, final_model="best_val"), VAL_LONG),
    (None, two, dict(PRODA, return_operand_stats=True), STATS),
    (None, eight, dict(n_cls=5, n_prompt=4, one_call=True, val=VAL), "f: " + C_LT_G),
    (None, eight, dict(n_cls=9, n_prompt=4, one_call=True, val=VAL), P_LT_G),
    (None, two, dict(PRODA, one_call=True, val=VAL), ONE_CALL),
    (None, two, dict(PRODA, val=VAL, return_operand_stats=True), VAL_LONG),
    # CoCoOp
    (None, (2, 0), dict(n_cls=5), TYPE),
    (None, eight, dict(n_cls=5), "f: " + C_LT_G),
    (None, two, dict(n_cls=5, one_call=True), ONE_CALL),
    (None, two, dict(n_cls=5, val=VAL), VAL_LONG),
    (None, two, dict(n_cls=5, final_model="best_val"), VAL_LONG),
    (None, two, dict(n_cls=5, return_operand_stats=True), STATS),
    (None, eight, dict(n_cls=5, one_call=True, val=VAL), "f: " + C_LT_G),
    (None, two, dict(n_cls=5, one_call=True, val=VAL), ONE_CALL),
    # the block fits (vptfit, maplefit, promptsrcfit): no class count, longer one-call and statistics sentences
    ("block", (2, 0), {}, TYPE),
    ("block", two, dict(one_call=True), ONE_CALL + " around one all-gather"),
    ("block", two, dict(val=VAL), VAL_LONG),
    ("block", two, dict(final_model="best_val"), VAL_LONG),
    ("block", two, dict(return_operand_stats=True), STATS + ": they are per rank"),
    ("block", two, dict(one_call=True, val=VAL, final_model="best_val", return_operand_stats=True), ONE_CALL + " around one all-gather"),
    ("block", two, dict(val=VAL, return_operand_stats=True), VAL_LONG),
]


@pytest.mark.parametrize("family,sh,facts,text", REFUSALS)
def test_check_refuses_with_the_family_s_text_in_the_family_s_order(family, sh, facts, text):
    with pytest.raises(ValueError) as e:
        shard.check("f", sh() if callable(sh) else sh, family, **facts)
    assert str(e.value) == text


def test_check_passes_what_every_family_takes_and_coopfit_keeps_the_names():
    for family, facts in (("coop", COOP), (None, PRODA), (None, dict(n_cls=5)), ("block", {})):
        shard.check("f", two(), family, **facts)
    shard.check("f", shard.Shard(5, 4, shard.LocalGather(5)), n_cls=5, n_prompt=5)               # C == G and P == G split
    assert (coopfit.Shard, coopfit.LocalGather, coopfit.shard_classes, coopfit.shard_states) == \
        (shard.Shard, shard.LocalGather, shard.shard_classes, shard.shard_states)
    with pytest.raises(ValueError) as e:
        shard.shard_classes(5, 8, 3)
    assert str(e.value) == C_LT_G
    with pytest.raises(ValueError) as e:
        shard.check_batch("f", shard.Shard(4, 1, shard.LocalGather(4)), 6)
    assert str(e.value) == "f: a batch of B=6 images does not split over G=4 ranks (B must be a multiple of G; ragged batches are not sharded)"


# ------------------------------------------------------------------------------------------------------------------------ the driver
class Stub:
    """A fit state as the driver sees it: a shard, a step counter, phases that log ``(rank, phase)``."""

    def __init__(self, sh, log, n_phases=3):
        self.shard, self.steps, self.log, self.n_phases = sh, 0, log, n_phases
        shard.file_state(sh, self)

    def phases(self, report=None):
        for k in range(self.n_phases):
            self.log.append((self.shard.rank, k))
            if k + 1 < self.n_phases:
                yield
        if report is not None:
            report["rank"] = self.shard.rank


def world(G, log, gather=None):
    gather = shard.LocalGather(G) if gather is None else gather
    return [Stub(shard.Shard(G, r, gather), log) for r in range(G)]


def test_run_phases_is_rank_major_within_a_phase_and_stops_when_all_end():
    log = []

    def gen(rank):
        for k in range(3):
            log.append((rank, k))
            yield
    shard.run_phases([gen(r) for r in range(3)])
    assert log == [(r, k) for k in range(3) for r in range(3)]


def test_world_states_wants_one_state_per_rank():
    lg, log = shard.LocalGather(3), []
    s0 = Stub(shard.Shard(3, 0, lg), log)
    with pytest.raises(ValueError) as e:
        shard.world_states(s0.shard, s0, "f")
    assert str(e.value) == "f: the LocalGather holds 1 of its 3 shard states; make one state per rank before the first step"
    rest = [Stub(shard.Shard(3, r, lg), log) for r in (1, 2)]
    assert shard.world_states(s0.shard, s0, "f") == [s0] + rest
    alone = Stub(shard.Shard(3, 1, lambda *a: None), log)                                      # an RCCL-style gather: the one state
    assert shard.world_states(alone.shard, alone, "f") == [alone] and shard.world_states(None, alone, "f") == [alone]


def test_the_first_state_that_steps_drives_until_new_states_are_filed():
    lg, log = shard.LocalGather(3), []
    states = world(3, log, lg)
    assert shard.drive(states[1].shard, states[1], "f") == states
    assert shard.drive(states[1].shard, states[1], "f") == states                              # the driver steps again
    with pytest.raises(ValueError) as e:
        shard.drive(states[2].shard, states[2], "f")
    assert str(e.value) == "f: under a LocalGather the step of rank 1's state steps every rank; rank 2's state must not be stepped as well"
    fresh = world(3, log, lg)                                                                  # a new set of states chooses its driver anew
    shard.drive(fresh[2].shard, fresh[2], "f")
    assert lg.driver is fresh[2]
    half = shard.LocalGather(2)
    s0 = Stub(shard.Shard(2, 0, half), log)
    with pytest.raises(ValueError, match="holds 1 of its 2 shard states"):                     # the incomplete world comes first
        shard.drive(s0.shard, s0, "f")
    assert half.driver is None
    alone = Stub(shard.Shard(3, 1, lambda *a: None), log)
    assert shard.drive(alone.shard, alone, "f") == [alone]                                     # under RCCL every rank steps its own state


def test_step_all_runs_every_rank_and_counts_the_peers():
    """Every fit's counters after a step: the driver counts its own step, as it does without ``shard``; ``step_all`` counts the peers'."""
    log = []
    states = world(3, log)
    drv = states[1]
    for n in (1, 2):
        shard.step_all(shard.drive(drv.shard, drv, "f"), drv, lambda s: s.phases())
        drv.steps += 1
        assert [s.steps for s in states] == [n, n, n]
    assert log == 2 * [(r, k) for k in range(3) for r in range(3)]
    shard.run_all(states[0].shard, states[0], "f", lambda s: s.phases())                       # a collective that is no step: anyone may enter
    assert [s.steps for s in states] == [2, 2, 2] and len(log) == 27 and states[0].shard.local.driver is drv
    alone = Stub(shard.Shard(3, 1, lambda *a: None), log)
    shard.step_all(shard.drive(alone.shard, alone, "f"), alone, lambda s: s.phases())
    assert alone.steps == 0                                                                    # its own step is the caller's to count


def test_report_all_returns_this_rank_s_report():
    log, lg = [], shard.LocalGather(3)
    state = shard.shard_states(lambda sh: Stub(sh, log), shard.Shard(3, 2, lg))
    report = shard.report_all(state.shard, state, "f", lambda s, r: s.phases(r))
    assert state is lg.states[2] and report == {"rank": 2} and log == [(r, k) for k in range(3) for r in range(3)]
    assert [s.steps for s in lg.states] == [0, 0, 0] and lg.driver is None
