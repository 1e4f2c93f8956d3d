"""CPU checks of the fit states' shared optimiser plumbing (clip_calibration_amd/fitoptim.py): every refusal that moved there with the
full text it has always had -- the strings below were recorded from ``coopfit``, ``prodafit``, ``cocoopfit``, ``vptfit``, ``maplefit``
and ``promptsrcfit`` before their copies were folded into ``fitoptim`` --, through the entry points that raise them wherever those need no
device.  ``scaler_state`` on a constructed state needs one: that test alone is marked ``gpu``."""
import pytest

import cocoopfit_ref
import coopfit_ref
import prodafit_ref
import vptfit_ref

from clip_calibration_amd import cocoopfit, coopfit, fitloop, fitoptim, maplefit, prodafit, promptsrcfit, vptfit  # noqa: E402
from clip_calibration_amd.model import build_model  # noqa: E402

ONE_CALL = "{who}: one_call=True with optimizer='adam': the one-call steps stay SGD"
BELONGS = "{who}: grad_scale='dynamic' belongs to a fit ({state}, {fit}); one gradient needs a number"
STATIC = "{state}.scaler_state: the state was made with a static grad_scale=256.0"
# (who, state, fit) of the six gradient entry points
ENTRIES = [("context_gradient", "CoOpFitState", "fit_context"), ("context_gradient", "ProDAFitState", "fit_context"),
           ("gradients", "CoCoOpFitState", "fit_prompt_learner"), ("prompt_gradient", "VPTFitState", "fit_prompts"),
           ("maplefit.gradients", "MaPLeFitState", "fit_prompt_learner"), ("promptsrcfit.gradients", "PromptSRCFitState", "fit_prompts")]


def raised(fn, *args, **kw) -> str:
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    return str(e.value)


@pytest.fixture(scope="module")
def cpu_model():
    return build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})


def test_private_names_have_one_home():
    for name in ("_check_grad_scale", "_is_dynamic", "_check_scaler", "_scale_args", "_BlockScaler", "_AdamBlock"):
        assert hasattr(fitoptim, name) and not hasattr(coopfit, name), name
    assert coopfit.DYNAMIC is fitoptim.DYNAMIC == "dynamic" and coopfit.DEFAULT_GRAD_SCALE == 4096.0
    for cls in (coopfit.CoOpFitState, prodafit.ProDAFitState, cocoopfit.CoCoOpFitState, vptfit.VPTFitState, maplefit.MaPLeFitState,
                promptsrcfit.PromptSRCFitState):
        assert issubclass(cls, fitoptim.Optimised) and cls.scaler_state is fitoptim.Optimised.scaler_state, cls


def test_one_call_with_adam():
    assert raised(fitloop.refuse_one_call, "S.step", "adam") == ONE_CALL.format(who="S.step")
    assert raised(fitloop.check_optimizer, "fit_prompts", "adam", 0.9, 0.0, False, 5e-4, one_call=True) == ONE_CALL.format(who="fit_prompts")
    assert raised(fitoptim.check_fit, "f", "adam", 0.9, 0.0, False, 5e-4, (0.9, 0.999), 1e-8, 256.0, None, one_call=True) == ONE_CALL.format(who="f")

    class State(fitoptim.Optimised):
        optimizer, _adam = "adam", object()
    assert raised(State()._no_one_call_adam, "CoCoOpFitState.step", True) == ONE_CALL.format(who="CoCoOpFitState.step")
    State()._no_one_call_adam("CoCoOpFitState.step", False)
    State._adam = None
    State()._no_one_call_adam("CoCoOpFitState.step", True)


def test_dynamic_scale_at_a_gradient_entry_point(cpu_model):
    for who, state, fit in ENTRIES:
        assert raised(fitoptim.static_grad_scale, who, "dynamic", state, fit) == BELONGS.format(who=who, state=state, fit=fit)
    assert fitoptim.static_grad_scale("f", 256, "S", "fit") == 256.0 and isinstance(fitoptim.static_grad_scale("f", 256, "S", "fit"), float)
    assert raised(fitoptim.static_grad_scale, "f", 3.0, "S", "fit") == "f: grad_scale=3.0 must be a power of two (the scaling has to be exact)"
    assert raised(fitoptim.static_grad_scale, "f", "auto", "S", "fit") == "f: grad_scale='auto' must be a power of two or 'dynamic'"
    # the entry points themselves
    c = coopfit_ref.make_case("tiny", 3, 4, 2, False)
    got = raised(coopfit.context_gradient, cpu_model, c["ids"], c["ctx"], c["feats"], c["labels"], grad_scale="dynamic")
    assert got == BELONGS.format(who="context_gradient", state="CoOpFitState", fit="fit_context")
    p = prodafit_ref.make_case("tiny", 3, 4, 8, 4, 2)
    got = raised(prodafit.context_gradient, cpu_model, p["ids"], p["ctx"], p["feats"], p["labels"], grad_scale="dynamic")
    assert got == BELONGS.format(who="context_gradient", state="ProDAFitState", fit="fit_context")
    cc = cocoopfit_ref.make_case("tiny", 3, 4, 2)
    got = raised(cocoopfit.gradients, cpu_model, cc["ids"], cc["params"], cc["feats"], cc["labels"], grad_scale="dynamic")
    assert got == BELONGS.format(who="gradients", state="CoCoOpFitState", fit="fit_prompt_learner")
    v = vptfit_ref.make_case("tiny", 2, 2, 2, 3)
    vm = build_model(dict(v["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0})
    got = raised(vptfit.prompt_gradient, vm, v["prompts"], v["images"], v["labels"], v["text"], grad_scale="dynamic")
    assert got == BELONGS.format(who="prompt_gradient", state="VPTFitState", fit="fit_prompts")
    got = raised(maplefit.gradients, None, None, None, None, None, grad_scale="dynamic")      # the first of its checks
    assert got == BELONGS.format(who="maplefit.gradients", state="MaPLeFitState", fit="fit_prompt_learner")
    got = raised(promptsrcfit.gradients, None, None, None, None, None, None, grad_scale="dynamic")
    assert got == BELONGS.format(who="promptsrcfit.gradients", state="PromptSRCFitState", fit="fit_prompts")


def test_scale_args_and_scaler():
    assert fitoptim._scale_args("f", 256.0, None) == (False, 256.0, None)
    dynamic, gs, cfg = fitoptim._scale_args("f", "dynamic", {"init_scale": 4})
    assert dynamic and gs is None and cfg == {"init_scale": 4.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000}
    assert raised(fitoptim._scale_args, "f", 256.0, {}) == "f: scaler is an argument of grad_scale='dynamic'"
    options = "['backoff_factor', 'growth_factor', 'growth_interval', 'init_scale']"
    assert raised(fitoptim._check_scaler, "f", [1]) == f"f: scaler must be a dict of {options} or None"
    assert raised(fitoptim._check_scaler, "f", {"growth": 2.0}) == f"f: scaler has no option 'growth' (one of {options})"
    assert raised(fitoptim._check_scaler, "f", {"init_scale": 3.0}) == ("f: scaler['init_scale']=3.0 must be a finite, positive power of two of fp32's range "
                                                                         "(the scaling has to be exact)")
    assert raised(fitoptim._check_scaler, "f", {"growth_factor": 0.5}) == "f: scaler growth_factor=0.5 (>= 1), backoff_factor=0.5 (<= 1)"
    assert raised(fitoptim._check_scaler, "f", {"growth_interval": 2.5}) == "f: scaler growth_interval=2.5 must be an integer >= 1"


def test_check_fit_keeps_the_drivers_order():
    args = ("adam", 0.9, 0.0, False, 5e-4, (0.9, 0.999), 1e-8)
    assert fitoptim.check_fit("f", *args, 256.0, None) == (False, 256.0, None)
    # the optimiser's refusals come first, then the hook, then the loss scale's
    assert raised(fitoptim.check_fit, "f", "lion", *args[1:], "auto", None) == "f: optimizer='lion' must be one of ('sgd', 'adam', 'adamw')"
    assert raised(fitoptim.check_fit, "f", *args, "auto", None, shard=object()) == "f: shard with optimizer='adam': the class-sharded fit stays SGD"

    def hook():
        raise ValueError("between")
    assert raised(fitoptim.check_fit, "f", *args, "auto", None, between=hook) == "between"
    assert raised(fitoptim.check_fit, "f", *args, "auto", None) == "f: grad_scale='auto' must be a power of two or 'dynamic'"


def test_head_scale_rows_and_sgd_tuple_off_the_device():
    class State(fitoptim.Optimised):
        _who = "S"
    st = State()
    st._init_optimiser("S", 4.6052, 0.9, 0, True, 5e-4, 256, None)
    assert (st.dynamic, st._head_scale, st.optimizer) == (False, 256.0, "sgd")
    assert st._sgd == (0.9, 0.0, 5e-4, 1) and [type(x) for x in st._sgd] == [float, float, float, int]
    st._scale_rows(object())          # static: nothing is touched
    assert raised(st.scaler_state) == "S.scaler_state: the state was made with a static grad_scale=256.0"
    dyn = State()
    dyn._init_optimiser("S", 4.6052, 0.9, 0.0, False, 5e-4, "dynamic", None, "adamw")
    assert (dyn.dynamic, dyn.grad_scale, dyn._head_scale, dyn.optimizer) == (True, None, 1.0, "adamw") and dyn._sgd == (0.0, 0.0, 5e-4, 0)
    for name in ("CoOpFitState", "ProDAFitState", "CoCoOpFitState", "VPTFitState", "MaPLeFitState", "PromptSRCFitState"):
        st._who = name
        assert raised(st.scaler_state) == STATIC.format(state=name)


@pytest.mark.gpu
def test_scaler_state_of_a_static_state():
    m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"}).cuda()
    c, p, cc, v = (coopfit_ref.make_case("tiny", 3, 4, 2, False), prodafit_ref.make_case("tiny", 3, 4, 8, 4, 2), cocoopfit_ref.make_case("tiny", 3, 4, 2),
                   vptfit_ref.make_case("tiny", 2, 2, 2, 3))
    vm = build_model(dict(v["sd"]), {"trainer": "VPT", "vision_depth": 2, "vision_ctx": 2, "language_depth": 0, "language_ctx": 0}).cuda()
    states = [coopfit.CoOpFitState(m, c["ids"], c["ctx"], grad_scale=256.0), prodafit.ProDAFitState(m, p["ids"], p["ctx"], grad_scale=256.0),
              cocoopfit.CoCoOpFitState(m, cc["ids"], cc["params"], grad_scale=256.0),
              vptfit.VPTFitState(vm, v["text"].cuda(), prompts=v["prompts"], grad_scale=256.0)]
    for st, name in zip(states, ("CoOpFitState", "ProDAFitState", "CoCoOpFitState", "VPTFitState")):
        assert raised(st.scaler_state) == STATIC.format(state=name)
    dyn = coopfit.CoOpFitState(m, c["ids"], c["ctx"], grad_scale="dynamic", scaler={"init_scale": 256.0})
    assert dyn.scaler_state() == {"scale": 256.0, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 0, "found_inf": 0}
    assert dyn.buf is not None and dyn.steps == 0 and dyn._adam is None
