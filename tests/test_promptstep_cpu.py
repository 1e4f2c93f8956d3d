"""The one-call training step of CoOp, KgCoOp and ProGrad has one body behind four entry points (static or dynamic loss scale, the
class token at the end or placed): every one of them refuses the same single-fault calls, before anything is launched, with the codes
the four separate bodies answered before they were merged.

No device is needed: the handle's text weights are bound to an address that only a kernel would read, so a call that passes every check
reaches its first launch and answers CLIPMI_ERR_HIP -- and a call that is refused late, behind a launch, would answer that too."""
import ctypes
import math

import pytest
import torch

from clip_calibration_amd import _lib, synthetic as syn
from clip_calibration_amd.model import build_model

A, S, W, HIP = _lib.ERR_ARG, _lib.ERR_SHAPE, _lib.ERR_WORKSPACE, _lib.ERR_HIP
PATHS = ("static", "scaled", "placed", "scaled_placed")
P = ctypes.c_void_p(4096)
ODD = ctypes.c_void_p(4096 + 8)

# fault -> the codes of (static, scaled, placed, scaled_placed) as the library built from the parent commit answered them
# (tools/build_prev_lib.sh, CLIPMI_LIBRARY, then `python tests/test_promptstep_cpu.py`); None: the path does not take the argument.
# CLIPMI_ERR_HIP in the first column: the parent's unplaced static step refused the head's and the step's arguments only behind the
# tower's forward, which has no device to run on here.  That is the one thing that changes: those refusals now come before the first
# launch, with the code the parent's placed static step (the same head and the same step, checked up front) gives the same fault.
PARENT = {
    'm': (A, A, A, A),
    'wt': (A, A, A, A),
    'prompts': (A, A, A, A),
    'ctx': (A, A, A, A),
    'eot': (A, A, A, A),
    'feats': (HIP, A, A, A),
    'labels': (HIP, A, A, A),
    'lr': (A, A, A, A),
    'losses': (A, A, A, A),
    'ws': (A, A, A, A),
    'stash': (A, A, A, A),
    'lens': (None, None, A, A),
    'B = 0': (S, S, S, S),
    'n_prompts = 1': (S, S, S, S),
    'bad mode': (A, A, A, A),
    'ld short of E': (HIP, S, S, S),
    'kgcoop without teacher': (HIP, A, A, A),
    'kgcoop w < 0': (HIP, A, A, A),
    'scale not finite': (HIP, A, A, A),
    'momentum without buffer': (HIP, A, A, A),
    'nesterov without momentum': (HIP, A, A, A),
    'workspace one byte short': (W, W, W, W),
    'workspace misaligned': (A, A, A, A),
    'state': (None, A, None, A),
    'state misaligned': (None, A, None, A),
    'growth_factor': (None, A, None, A),
    'backoff_factor': (None, A, None, A),
    'growth_interval': (None, A, None, A),
}
EXPECTED = {name: (row[2] if row[0] == HIP else row[0],) + row[1:] for name, row in PARENT.items()}


def _bound(geom="tiny"):
    m = build_model(dict(syn.synthetic_state_dict(geom, seed=0)), {"trainer": "CoOp"})
    m._ensure_handle()
    layers = int(m.geometry.transformer_layers)
    blocks = (_lib.BlockWeights * layers)()
    for b in blocks:
        for name in ("ln1_g", "ln1_b", "w_qkv", "b_qkv", "w_out", "b_out", "ln2_g", "ln2_b", "w_fc", "b_fc", "w_proj", "b_proj"):
            setattr(b, name, 4096)
    tw = _lib.TextWeights(4096, 4096, 4096, 4096, 4096, blocks)
    assert _lib.lib.clipmi_set_text_weights(m._handle, ctypes.byref(tw)) == _lib.OK
    dblocks = (_lib.BlockDgrad * layers)(*[_lib.BlockDgrad(4096, 4096, 4096, 4096) for _ in range(layers)])
    return m, (blocks, tw, dblocks, _lib.TextDgrad(4096, dblocks))


def _call(path, h, dgrad, E, **over):
    """One call of the path's symbol on arguments that pass every check, but for what `over` replaces."""
    lib = _lib.lib
    a = dict(m=h, wt=ctypes.byref(dgrad), prompts=P, ctx=P, buf=None, eot=P, feats=P, labels=P, lr=P, losses=P, ws=P, stash=P, lens=P, state=P, teacher=None,
             C=3, B=8, ld=E, mode=_lib.PROMPT_COOP, w=8.0, scale=100.0, momentum=0.0, nesterov=0, growth=2.0, backoff=0.5, interval=2000, short=0)
    a.update(over)
    scaled, placed = "scaled" in path, "placed" in path
    sizer = getattr(lib, "clipmi_prompt_train_step" + ("_scaled" if scaled else "") + ("_placed" if placed else "") + "_bytes")
    ws_bytes = sizer(h, 3, 16, 8, a["mode"] if a["mode"] in (0, 1, 2) else 0, 4, 0) - 1 if a["short"] else 1 << 40
    head = (a["m"], a["wt"], a["prompts"], _lib.F16, a["ctx"], a["buf"], 4, 0) + ((1, a["lens"]) if placed else ()) + (
        a["eot"], a["C"], 16, a["feats"], a["ld"], a["labels"], a["B"], a["scale"])
    tail = (a["ws"], ws_bytes, a["stash"], 1 << 40, None)
    sgd = (a["momentum"], 0.0, 5e-4, a["nesterov"])
    if scaled:
        fn = lib.clipmi_prompt_train_step_scaled_placed if placed else lib.clipmi_prompt_train_step_scaled
        return fn(*head, a["state"], a["growth"], a["backoff"], a["interval"], a["mode"], a["teacher"], a["w"], a["lr"], *sgd, a["losses"], None, *tail)
    fn = lib.clipmi_prompt_train_step_placed if placed else lib.clipmi_prompt_train_step
    return fn(*head, 256.0, a["mode"], a["teacher"], a["w"], 1.0, 1.0, a["lr"], 1, *sgd, a["losses"], None, None, None, *tail)


def faults():
    """name -> (the arguments replaced, the paths that take them)"""
    t = {n: ({n: None}, PATHS) for n in ("m", "wt", "prompts", "ctx", "eot", "feats", "labels", "lr", "losses", "ws", "stash")}
    t["lens"] = ({"lens": None}, ("placed", "scaled_placed"))
    t.update({
        "B = 0": ({"B": 0}, PATHS), "n_prompts = 1": ({"C": 1}, PATHS), "bad mode": ({"mode": 5}, PATHS),
        "ld short of E": ({"ld": 1}, PATHS),                                   # the head's arguments alone are bad
        "kgcoop without teacher": ({"mode": _lib.PROMPT_KGCOOP}, PATHS), "kgcoop w < 0": ({"mode": _lib.PROMPT_KGCOOP, "teacher": P, "w": -1.0}, PATHS),
        "scale not finite": ({"scale": math.inf}, PATHS), "momentum without buffer": ({"momentum": 0.9}, PATHS),
        "nesterov without momentum": ({"nesterov": 1}, PATHS), "workspace one byte short": ({"short": 1}, PATHS), "workspace misaligned": ({"ws": ODD}, PATHS)})
    both = ("scaled", "scaled_placed")
    t.update({"state": ({"state": None}, both), "state misaligned": ({"state": ctypes.c_void_p(4098)}, both), "growth_factor": ({"growth": 0.0}, both),
              "backoff_factor": ({"backoff": math.nan}, both), "growth_interval": ({"interval": 0}, both)})
    return t


def codes():
    m, keep = _bound()
    E = int(m.geometry.embed_dim)
    return {name: tuple(_call(p, m._handle, keep[3], E, **over) if p in paths else None for p in PATHS) for name, (over, paths) in faults().items()}


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a device a call that passes the checks would run on fake weights")
def test_four_paths_refuse_the_same_faults_with_the_parents_codes():
    got = codes()
    assert set(got) == set(EXPECTED)
    assert [n for n, row in PARENT.items() if row[0] == HIP] == ["feats", "labels", "ld short of E", "kgcoop without teacher", "kgcoop w < 0", "scale not finite",
                                                                 "momentum without buffer", "nesterov without momentum"]
    for name, want in EXPECTED.items():
        assert got[name] == want, (name, got[name], want, _lib.last_error())
    assert all(c in (A, S, W, None) for row in got.values() for c in row)      # never a launch: HIP is what a launch answers here


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a device a call that passes the checks would run on fake weights")
def test_a_call_that_passes_reaches_the_launch_and_unbound_weights_come_last():
    m, keep = _bound()
    E = int(m.geometry.embed_dim)
    for p in PATHS:
        assert _call(p, m._handle, keep[3], E) == HIP, p                       # every check passed: the first launch finds no device
    fresh = build_model(dict(syn.synthetic_state_dict("tiny", seed=0)), {"trainer": "CoOp"})
    fresh._ensure_handle()
    for p in PATHS:
        assert _call(p, fresh._handle, keep[3], E) == _lib.ERR_STATE, p
        assert _call(p, fresh._handle, keep[3], E, feats=None) == A and _call(p, fresh._handle, keep[3], E, momentum=0.9) == A, p


if __name__ == "__main__":                                                     # the recording run: CLIPMI_LIBRARY names the parent's build
    for name, row in codes().items():
        print(f"    {name!r}: {row},")
