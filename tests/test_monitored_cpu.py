"""``fitmonitor.Monitored``, the one monitor mix-in of the nine ``*FitState`` classes, and ``History.val_set``, the one cache of a
cached-feature validation set, without a GPU and without a library call: which methods every state inherits, the two public argument
orders of ``start_monitor``, what a state that never validated answers, the cache's key, and the fit functions' refusals with the texts
they had before they shared their checks."""
import inspect

import numpy as np
import pytest
import torch

import cocoopfit_ref
import coopfit_ref
import prodafit_ref
from clip_calibration_amd import adapterfit, cocoopfit, coopfit, fitloop, fitmonitor, maplefit, prodafit, promptsrcfit, taskresfit, vptfit
from clip_calibration_amd.model import build_model

CACHED = [(coopfit.CoOpFitState, "best_context"), (adapterfit.AdapterFitState, "best_weights"), (taskresfit.TaskResFitState, "best_residuals"),
          (cocoopfit.CoCoOpFitState, "best_params"), (prodafit.ProDAFitState, "best_params")]
IMAGE = [(vptfit.VPTFitState, "best_prompts"), (maplefit.MaPLeFitState, "best_params"), (promptsrcfit.PromptSRCFitState, "best_params")]
STATES = CACHED + IMAGE       # KgCoOp and ProGrad train on CoOpFitState: the ninth driver has no class of its own
ids = [cls.__name__ for cls, _ in STATES]


@pytest.mark.parametrize("cls,best", STATES, ids=ids)
def test_every_state_takes_the_monitor_surface_from_the_mix_in(cls, best):
    assert issubclass(cls, fitmonitor.Monitored) and cls._who == cls.__name__
    for name in ("monitor", "monitor_records", "_monitor_for", "_best_block"):
        assert getattr(cls, name) is getattr(fitmonitor.Monitored, name), name
    assert "validate" in vars(cls) and best in vars(cls)
    if (cls, best) in IMAGE:       # the image-tower states share one _master, over the name of their block
        assert cls._master is vptfit._BlockFitState._master and hasattr(cls, "_master_name") and issubclass(cls, fitmonitor.ImageMonitored)
    else:
        assert "_master" in vars(cls)
    assert coopfit.CoOpFitState.val_logits is fitmonitor.Monitored.val_logits
    assert cocoopfit.CoCoOpFitState.val_row_results is fitmonitor.Monitored.val_row_results


@pytest.mark.parametrize("cls,best", STATES, ids=ids)
def test_the_two_public_orders_of_start_monitor(cls, best):
    p = inspect.signature(cls.start_monitor).parameters
    tail = ("select", "val_criterion") if (cls, best) in CACHED else ("val_criterion", "select")
    assert tuple(p) == ("self", "slots", "val_bins") + tail
    assert p["slots"].default is inspect.Parameter.empty
    assert (p["val_bins"].default, p["select"].default, p["val_criterion"].default) == (10, False, "accuracy")


@pytest.mark.parametrize("cls,best", STATES, ids=ids)
def test_a_state_that_never_validated(cls, best):
    st = cls.__new__(cls)
    got, want = st.monitor(), fitmonitor.empty_monitor()
    assert set(got) == set(want) and got["records"] == [] and got["best_epoch"] is None
    for k in ("accuracy", "nll", "ece", "bins"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype
    with pytest.raises(ValueError) as e:
        st.monitor_records()
    assert str(e.value).startswith(f"{cls.__name__}.monitor_records: nothing has been validated")
    with pytest.raises(ValueError) as e:
        getattr(st, best)()
    assert str(e.value).startswith(f"{cls.__name__}.{best}") and "the monitor does not select (start_monitor(..., select=True))" in str(e.value)


def test_the_history_classes_and_the_before_first_validate_rule():
    want = {coopfit.CoOpFitState: (fitmonitor.Monitor, True), adapterfit.AdapterFitState: (fitmonitor.Monitor, True),
            taskresfit.TaskResFitState: (fitmonitor.Monitor, True), cocoopfit.CoCoOpFitState: (fitmonitor.ImageMonitor, False),
            prodafit.ProDAFitState: (fitmonitor.History, False), vptfit.VPTFitState: (fitmonitor.ImageMonitor, False),
            maplefit.MaPLeFitState: (fitmonitor.ImageMonitor, False), promptsrcfit.PromptSRCFitState: (fitmonitor.ImageMonitor, False)}
    for cls, (history, summary) in want.items():
        assert cls._history is history and cls._unseen_summary is summary, cls.__name__


def test_the_set_cache_goes_by_versions_types_and_label_objects(monkeypatch):
    monkeypatch.setattr(fitloop, "_need_gpu", lambda t, name: None)      # the cache itself runs on host tensors
    h = fitmonitor.History.__new__(fitmonitor.History)
    h.val = None
    made = []

    def prepare(f):
        made.append(f.dtype)
        return f.float() * 2

    f, labels = torch.randn(5, 8), [0, 1, 2, 0, 1]
    a, la, fresh = h.val_set("who", f, labels, 8, 3, prepare)
    assert fresh and len(made) == 1 and torch.equal(a, f * 2) and la.dtype == torch.int64 and la.tolist() == labels
    b, lb, fresh = h.val_set("who", f, labels, 8, 3, prepare)
    assert not fresh and len(made) == 1 and b is a and lb is la                 # the same tensor twice: one preparation
    labels[0] = 2                                                               # a list changed in place keeps its first upload
    _, lc, fresh = h.val_set("who", f, labels, 8, 3, prepare)
    assert not fresh and len(made) == 1 and lc is la and lc.tolist() == [0, 1, 2, 0, 1]
    f.add_(0)                                                                   # a bumped version: prepared again, labels uploaded again
    _, ld, fresh = h.val_set("who", f, labels, 8, 3, prepare)
    assert fresh and len(made) == 2 and ld.tolist() == [2, 1, 2, 0, 1]
    half = f.half()
    h.val_set("who", half, labels, 8, 3, prepare)
    assert made == [torch.float32, torch.float32, torch.float16]
    # a changed dtype at equal address, shape and strides (in elements): two preparations
    raw = torch.zeros(5, 8, dtype=torch.int32)
    h.val, made[:] = None, []
    h.val_set("who", raw.view(torch.float32), labels, 8, 3, prepare)
    as_int = raw.view(torch.float32).view(torch.int32)
    assert as_int.data_ptr() == raw.data_ptr() and as_int._version == raw.view(torch.float32)._version
    h.val_set("who", as_int, labels, 8, 3, prepare)
    assert made == [torch.float32, torch.int32]
    lt = torch.tensor([0, 1, 2, 0, 1])                                          # a label tensor is uploaded again when its version moves
    h.val_set("who", f, lt, 8, 3, prepare)
    lt[0] = 1
    _, le, fresh = h.val_set("who", f, lt, 8, 3, prepare)
    assert fresh and le.tolist() == [1, 1, 2, 0, 1]
    with pytest.raises(ValueError, match=r"who: val_features \(5, 7\) must be \[N_val >= 1, E = 8\]"):
        h.val_set("who", torch.zeros(5, 7), labels, 8, 3, prepare)
    with pytest.raises(ValueError, match="5 validation rows need 5 labels"):
        h.val_set("who", torch.zeros(5, 8), [0, 1], 8, 3, prepare)


def test_the_device_check_of_the_set_cache():
    h = fitmonitor.History.__new__(fitmonitor.History)
    h.val = None
    with pytest.raises(RuntimeError, match="`val_features` must be a tensor on the GPU"):
        h.val_set("who", torch.zeros(5, 8), [0] * 5, 8, 3, lambda f: f)


def _fits():
    """(who, a call of the fit function on host tensors, E) for the five cached-feature fit functions."""
    g = torch.Generator().manual_seed(0)
    E, C, N = 8, 3, 6
    f, y = torch.randn(N, E, generator=g), torch.arange(N) % C
    text, w1, w2 = torch.randn(C, E, generator=g), torch.randn(2, E, generator=g), torch.randn(E, 2, generator=g)
    m = build_model(dict(coopfit_ref.state_dict("tiny")), {"trainer": "CoOp"})
    c, cc, d = coopfit_ref.make_case("tiny", C, 4, 2), cocoopfit_ref.make_case("tiny", C, 4, 2), prodafit_ref.make_case("tiny", C, 4, 4, 2, 2)
    Em = c["feats"].shape[1]
    return [("fit_context", lambda **k: coopfit.fit_context(c["feats"], c["labels"], m, c["ids"], c["ctx"], epochs=1, **k), Em),
            ("fit_adapter", lambda **k: adapterfit.fit_adapter(f, y, text, w1, w2, epochs=1, **k), E),
            ("fit_residuals", lambda **k: taskresfit.fit_residuals(f, y, text, epochs=1, **k), E),
            ("fit_prompt_learner", lambda **k: cocoopfit.fit_prompt_learner(cc["feats"], cc["labels"], m, cc["ids"], cc["params"], epochs=1, **k), Em),
            ("fit_context", lambda **k: prodafit.fit_context(d["feats"], d["labels"], m, d["ids"], d["ctx"], prompt_bs=2, epochs=1, **k), Em)]


def test_the_fit_functions_keep_their_refusals_word_for_word():
    """The expected texts are the ones the five functions raised while each spelled its checks out (or called ``check_args``)."""
    for who, call, E in _fits():
        val = (torch.zeros(4, E), torch.tensor([0, 1, 2, 0]))
        with pytest.raises(ValueError) as e:
            call(final_model="best_val")
        assert str(e.value) == f"{who}: final_model='best_val' needs val=(val_features, val_labels)"
        with pytest.raises(ValueError) as e:
            call(val=val, val_criterion="ece")
        assert str(e.value) == f"{who}: val_criterion='ece' must be one of ['accuracy', 'nll']"
        with pytest.raises(ValueError) as e:
            call(val=val[0])
        assert str(e.value) == f"{who}: val must be (val_features, val_labels)"
        with pytest.raises(ValueError) as e:
            call(val=(torch.zeros(4, E + 1), val[1]))
        assert str(e.value) == f"{who}: val_features must be a [N_val >= 1, E = {E}] tensor"
        with pytest.raises(RuntimeError, match="GPU"):      # everything about val was accepted
            call(val=val, final_model="best_val")


def test_returned_monitor_is_the_fit_functions_tail():
    class State:
        def monitor(self):
            return "monitor()"

    assert fitmonitor.returned_monitor(State(), True, 7, False) is None and fitmonitor.returned_monitor(State(), False, 7, False) is None
    assert fitmonitor.returned_monitor(State(), True, 7, True) == "monitor()"
    empty = fitmonitor.returned_monitor(State(), False, 7, True)
    assert empty["bins"].shape == (0, 3, 8) and empty["best_epoch"] is None and empty["records"] == []
    assert np.array_equal(empty["accuracy"], np.zeros(0))
