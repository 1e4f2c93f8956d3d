"""The three cached-feature fits through their C entry points (clipmi_taskres_train_step / clipmi_taskres_fit, clipmi_adapter_train_step /
clipmi_adapter_fit, clipmi_tempscale_batch / clipmi_tempscale_fit) at the shapes that cross every seam of their kernels and at ImageNet's
1000 classes, held element by element to the bound tests/cached_fit_ref.py derives (tests/test_cached_fit_ref_cpu.py holds an fp32
emulation to the same bound and shows seeded defects leaving it).  No tolerance here comes from the device or from a tensor's maximum.

Every input lies inside a NaN-patterned guard (the columns behind a strided feature or cosine row are NaN as well), labels sit in a buffer of
-7 and `order` in a buffer of out-of-range indices, every output and every updated tensor is sentinel-guarded, the workspace is a guarded
buffer of EXACTLY the floats the kernels carve (the call is told the bytes the sizing function returns; see ``_ws``), and every step is made twice.  The row losses are read as the loss history of a
fit with one row per batch at rate 0, the gradients from the momentum buffers of a first step, where the kernels leave them unrounded.
Every figure is printed on a line that starts with "cached-fits-parity:"; profiles/cached_fits_parity.txt is one run's lines."""
import numpy as np
import pytest
import torch

import cached_fit_ref as ref
from clip_calibration_amd import _lib
from test_gpu_glue_ops import Guarded, _assert_bits, _assert_within, _stream

pytestmark = pytest.mark.gpu

L = _lib.lib
RATIOS = {}
F = np.float32
F32 = torch.float32
NAN = float("nan")
BAD_INDEX = 1 << 30
B1, B2 = ref.ADAM["betas"]
EPS = ref.ADAM["eps"]
BIG_TASKRES, BIG_ADAPTER, BIG_TEMPSCALE = (257, 64, 1000), (3, 768, 192, 1000), (257, 1000)


def _f32(a):
    t = torch.as_tensor(np.array(a) if isinstance(a, np.ndarray) else a).float().contiguous()
    return Guarded(t.numel(), F32, t)


class _Labels:
    """int64 labels in the middle of a buffer of -7 (a label read from outside poisons the row)."""

    def __init__(self, y):
        y = torch.as_tensor(np.array(y))
        self.buf = torch.full((y.numel() + 16,), -7, dtype=torch.int64, device="cuda")
        self.buf[8:8 + y.numel()] = y.cuda()
        self.ptr = self.buf[8:].data_ptr()


class _Order:
    """int32 sample indices in the middle of a buffer of out-of-range indices (an index read from outside is no sample: NaN)."""

    def __init__(self, order):
        o = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32).reshape(-1))
        self.buf = torch.full((o.numel() + 16,), BAD_INDEX, dtype=torch.int32, device="cuda")
        self.buf[8:8 + o.numel()] = o.cuda()
        self.ptr = self.buf[8:].data_ptr()


def _rows(a, ld, perm=None):
    """[n, cols] in a guarded [n, ld] matrix whose columns behind `cols` are NaN; with ``perm`` row b lies at perm[b] (and order = perm reads it back)."""
    a = torch.from_numpy(np.array(a)).float()
    n, cols = a.shape
    wide = torch.full((n, ld), NAN)
    wide[torch.arange(n) if perm is None else torch.from_numpy(np.asarray(perm, np.int64)), :cols] = a
    return Guarded(n * ld, F32, wide)


def _scatter(y, perm):
    if perm is None:
        return np.array(y)
    out = np.empty_like(np.asarray(y))
    out[np.asarray(perm)] = y
    return out


def _ws(need, carve, misalign=0):
    """The workspace: the call is told the ``need`` bytes its sizing function reports, which rounds up to 256; the guard begins right behind
    the ``carve`` floats the source's layout comment lists (z | dz | loss | nf | nt; h | da | dh | z | loss; the pairs), so a write into the
    up to 252 bytes of rounding slack is seen as well (the slack lies inside the guard's own 256 bytes: no launch is handed less memory)."""
    assert need > 0 and need % 256 == 0 and 0 <= need - 4 * carve < 256
    return Guarded(carve + (1 if misalign else 0), F32)


def _perm(n, seed=5, epochs=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int32)


def _note(method, name, case, got, bound):
    want, tol = bound
    r = ref.ratio(got, want, tol)
    RATIOS[(method, name, str(case))] = r
    w, t = want.reshape(-1), torch.as_tensor(tol).expand(want.shape).reshape(-1)
    live = (w != 0) & torch.isfinite(t)
    med = float((t[live] / w[live].abs()).median())
    print(f"cached-fits-parity: {method:>9s} {name:>7s} {str(case):>44s} max err/bound {r:.4f}  median bound/|value| {med:.1e}")
    _assert_within(got, want, tol, f"{method} {case}: {name}")


def _same(a, b, what):
    for n in a:
        _assert_bits(a[n], b[n], f"{what}: {n}: two launches on the same input differ")


def _t32(*values):
    return torch.from_numpy(np.array(values, dtype=F))


def _mean32(rows):
    return _t32(rows.double().numpy().mean(dtype=np.float64))


# --------------------------------------------------------------------------------------------------------------------------- TaskRes
class TaskRes:
    """The buffers of one TaskRes problem; ``step`` and ``fit`` make one call each and leave (rc, guarded outputs)."""
    OUT = ("res", "s1", "s2", "loss")

    def __init__(self, f, y, base, r, ld_extra=0, perm=None):
        self.n, self.E = f.shape
        self.C = base.shape[0]
        self.ld = self.E + ld_extra
        self.feats, self.y = _rows(f, self.ld, perm), _Labels(_scatter(y, perm))
        self.base, self.res = _f32(base), _f32(r)
        self.s1, self.s2 = _f32(torch.zeros(self.C * self.E)), _f32(torch.zeros(self.C * self.E))
        self.init = torch.from_numpy(np.array(r)).float().reshape(-1)

    def step(self, lr=1.0, optimizer=0, momentum=0.0, wd=0.0, steps_done=0, short=0, misalign=0, ld=None, feats=None, y=None, rows=None):
        rows = self.n if rows is None else rows
        need = L.clipmi_taskres_train_workspace_bytes(rows, self.E, self.C)
        self.ws, self.lr, self.loss = _ws(need, 2 * rows * self.C + 2 * rows + self.C, misalign), _f32(torch.tensor([lr])), Guarded(1, F32)
        rc = L.clipmi_taskres_train_step((feats or self.feats).ptr, self.ld if ld is None else ld, (y or self.y).ptr, self.base.ptr, self.res.ptr,
                                         self.s1.ptr, self.s2.ptr, rows, self.E, self.C, ref.ALPHA, ref.S, self.lr.ptr, optimizer, steps_done, wd,
                                         momentum, 0.0, 0, B1, B2, EPS, self.loss.ptr, self.ws.ptr + misalign, need - short, _stream())
        torch.cuda.synchronize()
        return rc

    def fit(self, order, batch, epochs, lrs, optimizer=0, momentum=0.0, wd=0.0, drop_last=0):
        width = min(batch, self.n)
        need = L.clipmi_taskres_train_workspace_bytes(width, self.E, self.C)
        self.ws, self.lr, self.loss = _ws(need, 2 * width * self.C + 2 * width + self.C), _f32(torch.tensor(lrs)), Guarded(len(lrs), F32)
        self.order = None if order is None else _Order(order)
        rc = L.clipmi_taskres_fit(self.feats.ptr, self.ld, self.y.ptr, None if order is None else self.order.ptr, self.base.ptr, self.res.ptr,
                                  self.s1.ptr, self.s2.ptr, self.n, self.E, self.C, batch, epochs, drop_last, ref.ALPHA, ref.S, self.lr.ptr, optimizer,
                                  0, wd, momentum, 0.0, 0, B1, B2, EPS, self.loss.ptr, self.ws.ptr, need, _stream())
        torch.cuda.synchronize()
        return rc

    def values(self, what):
        for g, n in ((self.feats, "feats"), (self.base, "base"), (self.lr, "lr"), (self.ws, "workspace of exactly the reported bytes")):
            g.result(f"{what}: {n}")
        return {n: getattr(self, n).result(f"{what}: {n}") for n in self.OUT}


# (shape, ld - E, through `order`): one case with ld = E + 24, one through clipmi_taskres_fit's order
TASKRES_CASES = [((65, 70, 257), 24, False), ((257, 64, 1000), 0, False), ((3, 1024, 66), 0, True)]


def _taskres_once(case, **kw):
    """One step from the case's residuals, made twice: {res, s1, s2, loss}."""
    shape, ld_extra, via_order = case
    c = ref.taskres_case(shape)
    got = []
    for _ in range(2):
        perm = _perm(shape[0])[0] if via_order else None
        t = TaskRes(c["f"], c["y"], c["base"], c["r"], ld_extra, perm)
        if via_order:
            rc = t.fit(perm, shape[0], 1, [kw.get("lr", 1.0)], **{k: v for k, v in kw.items() if k != "lr"})
        else:
            rc = t.step(**kw)
        _lib.check(rc, f"taskres {case}")
        got.append(t.values(f"taskres {case}"))
    _same(got[0], got[1], f"taskres {case}")
    return got[0]


def _taskres_row_losses(case):
    """Every row as a batch of its own at rate 0: the loss history is the row losses, the residuals keep their bits."""
    shape, ld_extra, via_order = case
    c = ref.taskres_case(shape)
    perm = _perm(shape[0])[0] if via_order else None
    t = TaskRes(c["f"], c["y"], c["base"], c["r"], ld_extra, perm)
    _lib.check(t.fit(perm, 1, 1, [0.0] * shape[0]), f"taskres {case}: one row per batch")
    v = t.values(f"taskres {case}: one row per batch")
    _assert_bits(v["res"], t.init, "rate 0 keeps the residuals")
    return v["loss"]


@pytest.mark.parametrize("case", TASKRES_CASES, ids=str)
def test_taskres_step_within_bound(case):
    shape = case[0]
    C, E = shape[2], shape[1]
    bound = ref.taskres_bound(shape)
    r0 = torch.from_numpy(np.array(ref.taskres_case(shape)["r"])).reshape(-1)
    a, b = _taskres_once(case), _taskres_once(case, momentum=0.9)
    g = b["s1"]                                                      # the momentum buffer of a first step is the gradient itself
    _assert_bits(a["res"], b["res"], "a first step with and without a momentum")
    _assert_bits(a["loss"], b["loss"], "the loss with and without a momentum")
    _assert_bits(a["res"], r0 - g, "r' == fl(r - g) at lr 1")
    assert not a["s1"].any() and not a["s2"].any() and not b["s2"].any(), "SGD touched a state buffer it does not use"
    rows = _taskres_row_losses(case)
    _note("taskres", "rows", case, rows, bound["rows"])
    _note("taskres", "loss", case, a["loss"], bound["loss"])
    _assert_bits(a["loss"], _mean32(rows), "the batch loss is the float64 mean of the fp32 row losses")
    _note("taskres", "dr", case, g.reshape(C, E), bound["dr"])
    _note("taskres", "r_sgd", case, a["res"].reshape(C, E), bound["r_sgd"])
    adam = _taskres_once(case, optimizer=1, lr=ref.ADAM_LR)
    _note("taskres", "r_adam", case, adam["res"].reshape(C, E), bound["r_adam"])
    _assert_bits(adam["loss"], a["loss"], "the loss of the Adam step")


RAGGED_RATES = [0.01] * 3 + [0.005] * 3


def test_taskres_ragged_fit_equals_steps():
    """n = 257 in batches of 100 for two epochs through `order`: the last step of an epoch has 57 rows in a workspace sized for 100.  The
    fit leaves the bits of the same six steps made one at a time on gathered rows through clipmi_taskres_train_step."""
    shape = BIG_TASKRES
    c = ref.taskres_case(shape)
    order = _perm(shape[0], seed=9, epochs=2)
    kw = dict(momentum=0.9, wd=5e-4)
    fit = TaskRes(c["f"], c["y"], c["base"], c["r"])
    _lib.check(fit.fit(order, 100, 2, RAGGED_RATES, **kw), "taskres ragged fit")
    want = fit.values("taskres ragged fit")
    one = TaskRes(c["f"], c["y"], c["base"], c["r"])
    losses = []
    for step, (e, k) in enumerate((e, k) for e in range(2) for k in range(3)):
        idx = order[e, 100 * k:100 * k + 100]
        gathered = _rows(c["f"][idx], shape[1])
        _lib.check(one.step(lr=RAGGED_RATES[step], steps_done=step, feats=gathered, y=_Labels(c["y"][idx]), rows=len(idx), **kw), f"taskres step {step}")
        gathered.result(f"taskres step {step}: the gathered rows")
        losses.append(one.values(f"taskres step {step}")["loss"])
    got = one.values("taskres steps")
    assert torch.isfinite(want["res"]).all() and not torch.equal(want["res"], fit.init)
    for n in ("res", "s1", "s2"):
        _assert_bits(got[n], want[n], f"taskres: steps vs fit: {n}")
    _assert_bits(torch.cat(losses), want["loss"], "taskres: steps vs fit: losses")


@pytest.mark.parametrize("kind", ["label=C", "label=-1", "order=n"])
def test_taskres_bad_label_or_index_poisons_and_never_addresses(kind):
    """One bad label or sample index at 1000 classes: that row's loss and gradient are NaN, so the batch loss and -- every class sums over
    every row -- all residuals are NaN; every guard is intact."""
    shape = BIG_TASKRES
    c = ref.taskres_case(shape)
    y, order = np.array(c["y"]), np.arange(shape[0], dtype=np.int32)
    if kind == "order=n":
        order[130] = shape[0]
    else:
        y[130] = shape[2] if kind == "label=C" else -1
    t = TaskRes(c["f"], y, c["base"], c["r"])
    _lib.check(t.fit(order, shape[0], 1, [1.0]), f"taskres {kind}")
    v = t.values(f"taskres {kind}")
    assert torch.isnan(v["loss"]).all() and torch.isnan(v["res"]).all()
    # one row per batch at rate 0, the bad sample last: every earlier step's loss keeps the clean run's bits, the last is NaN
    last = np.concatenate([np.delete(np.arange(shape[0], dtype=np.int32), 130), order[130:131]])
    clean = TaskRes(c["f"], c["y"], c["base"], c["r"])
    _lib.check(clean.fit(np.concatenate([last[:-1], [130]]), 1, 1, [0.0] * shape[0]), f"taskres {kind}: clean rows")
    want = clean.values(f"taskres {kind}: clean rows")["loss"]
    t = TaskRes(c["f"], y, c["base"], c["r"])
    _lib.check(t.fit(last, 1, 1, [0.0] * shape[0]), f"taskres {kind}: rows")
    v = t.values(f"taskres {kind}: rows")
    assert torch.isfinite(want).all()
    _assert_bits(v["loss"][:-1], want[:-1], f"taskres {kind}: the rows before the bad one")
    assert torch.isnan(v["loss"][-1]) and torch.isnan(v["res"]).all()


def test_taskres_rejections_write_nothing():
    shape = (65, 70, 257)
    c = ref.taskres_case(shape)
    for kw, want in ((dict(short=1), _lib.ERR_WORKSPACE), (dict(misalign=4), _lib.ERR_ARG), (dict(ld=shape[1] - 1), _lib.ERR_SHAPE)):
        t = TaskRes(c["f"], c["y"], c["base"], c["r"])
        assert t.step(momentum=0.9, **kw) == want, kw
        v = t.values(f"taskres rejected {kw}")
        _assert_bits(v["res"], t.init, f"rejected {kw}: residuals")
        assert not v["s1"].any() and t.loss.untouched() and t.ws.untouched(), kw


# ---------------------------------------------------------------------------------------------------------------------- CLIP-Adapter
class Adapter:
    OUT = ("w1", "w2", "m1", "m2", "loss")

    def __init__(self, c, ld_extra=0, perm=None, y=None):
        f = c["f"]
        self.n, self.E = f.shape
        self.H, self.C = c["w1"].shape[0], c["T"].shape[0]
        self.ld = f.shape[1] + ld_extra
        self.feats, self.y = _rows(f, self.ld, perm), _Labels(_scatter(c["y"] if y is None else y, perm))
        self.text, self.w1, self.w2 = _f32(c["T"]), _f32(c["w1"]), _f32(c["w2"])
        self.m1, self.m2 = _f32(torch.zeros(c["w1"].size)), _f32(torch.zeros(c["w2"].size))
        self.init = {n: torch.from_numpy(np.array(c[n])).float().reshape(-1) for n in ("w1", "w2")}

    def step(self, lr=1.0, momentum=0.0, wd=0.0, first_step=1, short=0, misalign=0, ld=None, feats=None, y=None, rows=None):
        rows = self.n if rows is None else rows
        need = L.clipmi_adapter_train_workspace_bytes(rows, self.E, self.H, self.C)
        self.ws, self.lr, self.loss = _ws(need, rows * (self.E + 2 * self.H + self.C + 1), misalign), _f32(torch.tensor([lr])), Guarded(1, F32)
        rc = L.clipmi_adapter_train_step((feats or self.feats).ptr, self.ld if ld is None else ld, (y or self.y).ptr, self.text.ptr, self.w1.ptr,
                                         self.w2.ptr, self.m1.ptr, self.m2.ptr, rows, self.E, self.H, self.C, ref.RATIO, ref.S, self.lr.ptr,
                                         first_step, momentum, 0.0, wd, 0, self.loss.ptr, self.ws.ptr + misalign, need - short, _stream())
        torch.cuda.synchronize()
        return rc

    def fit(self, order, batch, epochs, lrs, momentum=0.0, wd=0.0, drop_last=0):
        width = min(batch, self.n)
        need = L.clipmi_adapter_train_workspace_bytes(width, self.E, self.H, self.C)
        self.ws, self.lr, self.loss = _ws(need, width * (self.E + 2 * self.H + self.C + 1)), _f32(torch.tensor(lrs)), Guarded(len(lrs), F32)
        self.order = None if order is None else _Order(order)
        rc = L.clipmi_adapter_fit(self.feats.ptr, self.ld, self.y.ptr, None if order is None else self.order.ptr, self.text.ptr, self.w1.ptr,
                                  self.w2.ptr, self.m1.ptr, self.m2.ptr, self.n, self.E, self.H, self.C, batch, epochs, drop_last, ref.RATIO, ref.S,
                                  self.lr.ptr, 1, momentum, 0.0, wd, 0, self.loss.ptr, self.ws.ptr, need, _stream())
        torch.cuda.synchronize()
        return rc

    def values(self, what):
        for g, n in ((self.feats, "feats"), (self.text, "text"), (self.lr, "lr"), (self.ws, "workspace of exactly the reported bytes")):
            g.result(f"{what}: {n}")
        return {n: getattr(self, n).result(f"{what}: {n}") for n in self.OUT}


# (shape, ld - E, through `order`)
ADAPTER_CASES = [((3, 768, 192, 1000), 0, False), ((2, 640, 160, 17), 8, False), ((5, 171, 48, 257), 0, True), ((257, 64, 16, 3), 0, False),
                 ((2, 3800, 64, 3), 0, False)]


def _adapter_once(case, **kw):
    shape, ld_extra, via_order = case
    c = ref.adapter_case(shape)
    got = []
    for _ in range(2):
        perm = _perm(shape[0])[0] if via_order else None
        t = Adapter(c, ld_extra, perm)
        rc = t.fit(perm, shape[0], 1, [kw.get("lr", 1.0)], **{k: v for k, v in kw.items() if k != "lr"}) if via_order else t.step(**kw)
        _lib.check(rc, f"adapter {case}")
        got.append(t.values(f"adapter {case}"))
    _same(got[0], got[1], f"adapter {case}")
    return got[0]


@pytest.mark.parametrize("case", ADAPTER_CASES, ids=str)
def test_adapter_step_within_bound(case):
    """The entries of dW1 / dW2 that depend on a unit whose float64 pre-activation lies within its own bound of zero are left out
    (cached_fit_ref.adapter_masks; tests/test_cached_fit_ref_cpu.py holds their share below adapterfit_ref.EXCLUDED_CAP); every other
    entry is inside the bound."""
    shape, ld_extra, via_order = case
    _, E, H, _ = shape
    c = ref.adapter_case(shape)
    bound = ref.adapter_bound(shape)
    a, b = _adapter_once(case), _adapter_once(case, momentum=0.9)
    for n, m in (("w1", "m1"), ("w2", "m2")):
        _assert_bits(a[n], b[n], f"{n}: a first step with and without a momentum")
        _assert_bits(a[n], torch.from_numpy(np.array(c[n])).reshape(-1) - b[m], f"{n}' == fl({n} - g) at lr 1")
        assert not a[m].any(), f"{m} touched without a momentum"
    perm = _perm(shape[0])[0] if via_order else None
    t = Adapter(c, ld_extra, perm)
    _lib.check(t.fit(perm, 1, 1, [0.0] * shape[0]), f"adapter {case}: one row per batch")
    v = t.values(f"adapter {case}: one row per batch")
    _assert_bits(v["w1"], t.init["w1"], "rate 0 keeps w1")
    _assert_bits(v["w2"], t.init["w2"], "rate 0 keeps w2")
    _note("adapter", "rows", case, v["loss"], bound["rows"])
    _note("adapter", "loss", case, a["loss"], bound["loss"])
    _assert_bits(a["loss"], _mean32(v["loss"]), "the batch loss is the float64 mean of the fp32 row losses")
    k1, k2 = ref.adapter_masks(shape)                                # from the float64 reference alone; the CPU test holds the cap
    _note("adapter", "dw1", case, b["m1"].reshape(H, E), ref.masked(bound["dw1"], k1))
    _note("adapter", "dw2", case, b["m2"].reshape(E, H), ref.masked(bound["dw2"], k2))
    _note("adapter", "w1", case, a["w1"].reshape(H, E), ref.masked(bound["w1"], k1))
    _note("adapter", "w2", case, a["w2"].reshape(E, H), ref.masked(bound["w2"], k2))


def test_adapter_refuses_the_first_shape_beyond_its_lds():
    """E = 3800 with H = 64 is exactly 64 KiB of LDS per sample (the last case above); H = 65 is the first shape refused: CLIPMI_ERR_SHAPE, nothing written."""
    rng = np.random.default_rng(3)
    E, H, C = 3800, 65, 3
    c = dict(f=rng.normal(size=(2, E)).astype(F), y=np.array([2, 0]), T=rng.normal(size=(C, E)).astype(F), w1=rng.normal(size=(H, E)).astype(F),
             w2=rng.normal(size=(E, H)).astype(F))
    t = Adapter(c)
    assert t.step(momentum=0.9) == _lib.ERR_SHAPE
    v = t.values("adapter E = 3800, H = 65")
    _assert_bits(v["w1"], t.init["w1"], "refused: w1")
    _assert_bits(v["w2"], t.init["w2"], "refused: w2")
    assert not v["m1"].any() and not v["m2"].any() and t.loss.untouched() and t.ws.untouched()


def test_adapter_ragged_fit_equals_steps():
    """n = 257 rows of the 1000-class problem's width in batches of 100 for two epochs through `order` (a last step of 57 rows in a workspace
    sized for 100): the bits of the same six steps made one at a time on gathered rows through clipmi_adapter_train_step."""
    _, E, H, C = BIG_ADAPTER
    n = 257
    c = dict(ref.adapter_case(BIG_ADAPTER))
    rng = np.random.default_rng(21)
    c["f"], c["y"] = rng.normal(size=(n, E)).astype(F), rng.integers(0, C, n)
    order = _perm(n, seed=9, epochs=2)
    kw = dict(momentum=0.9, wd=5e-4)
    fit = Adapter(c)
    _lib.check(fit.fit(order, 100, 2, RAGGED_RATES, **kw), "adapter ragged fit")
    want = fit.values("adapter ragged fit")
    one = Adapter(c)
    losses = []
    for step, (e, k) in enumerate((e, k) for e in range(2) for k in range(3)):
        idx = order[e, 100 * k:100 * k + 100]
        gathered = _rows(c["f"][idx], E)
        _lib.check(one.step(lr=RAGGED_RATES[step], first_step=int(step == 0), feats=gathered, y=_Labels(c["y"][idx]), rows=len(idx), **kw),
                   f"adapter step {step}")
        gathered.result(f"adapter step {step}: the gathered rows")
        losses.append(one.values(f"adapter step {step}")["loss"])
    got = one.values("adapter steps")
    assert torch.isfinite(want["w1"]).all() and not torch.equal(want["w1"], fit.init["w1"])
    for name in ("w1", "w2", "m1", "m2"):
        _assert_bits(got[name], want[name], f"adapter: steps vs fit: {name}")
    _assert_bits(torch.cat(losses), want["loss"], "adapter: steps vs fit: losses")


@pytest.mark.parametrize("kind", ["label=C", "label=-1", "order=n"])
def test_adapter_bad_label_or_index_poisons_and_never_addresses(kind):
    """One bad label or sample index at 1000 classes: the row's h, da, dh and loss are NaN, so the batch loss and -- every weight sums over
    every row -- both matrices are NaN; every guard is intact."""
    shape = BIG_ADAPTER
    c = ref.adapter_case(shape)
    y, order = np.array(c["y"]), np.arange(shape[0], dtype=np.int32)
    if kind == "order=n":
        order[1] = shape[0]
    else:
        y[1] = shape[3] if kind == "label=C" else -1
    t = Adapter(c, y=y)
    _lib.check(t.fit(order, shape[0], 1, [1.0]), f"adapter {kind}")
    v = t.values(f"adapter {kind}")
    assert torch.isnan(v["loss"]).all() and torch.isnan(v["w1"]).all() and torch.isnan(v["w2"]).all()
    # one row per batch at rate 0, the bad sample last: every earlier step's loss keeps the clean run's bits, the last is NaN
    last = np.array([0, 2, order[1]], np.int32)
    clean = Adapter(c)
    _lib.check(clean.fit(np.array([0, 2, 1], np.int32), 1, 1, [0.0] * 3), f"adapter {kind}: clean rows")
    want = clean.values(f"adapter {kind}: clean rows")["loss"]
    t = Adapter(c, y=y)
    _lib.check(t.fit(last, 1, 1, [0.0] * 3), f"adapter {kind}: rows")
    v = t.values(f"adapter {kind}: rows")
    assert torch.isfinite(want).all()
    _assert_bits(v["loss"][:-1], want[:-1], f"adapter {kind}: the rows before the bad one")
    assert torch.isnan(v["loss"][-1]) and torch.isnan(v["w1"]).all() and torch.isnan(v["w2"]).all()


def test_adapter_rejections_write_nothing():
    shape = (5, 171, 48, 257)
    c = ref.adapter_case(shape)
    for kw, want in ((dict(short=1), _lib.ERR_WORKSPACE), (dict(misalign=4), _lib.ERR_ARG), (dict(ld=shape[1] - 1), _lib.ERR_SHAPE)):
        t = Adapter(c)
        assert t.step(momentum=0.9, **kw) == want, kw
        v = t.values(f"adapter rejected {kw}")
        _assert_bits(v["w1"], t.init["w1"], f"rejected {kw}: w1")
        _assert_bits(v["w2"], t.init["w2"], f"rejected {kw}: w2")
        assert not v["m1"].any() and not v["m2"].any() and t.loss.untouched() and t.ws.untouched(), kw


# ----------------------------------------------------------------------------------------------------------------------- TempScaling
class TempScale:
    def __init__(self, c, y, ld_extra=0, perm=None):
        self.n, self.C = c.shape
        self.ld = self.C + ld_extra
        self.cos, self.y = _rows(c, self.ld, perm), _Labels(_scatter(y, perm))

    def batch(self, theta, order=None, rows=None, short=0, misalign=0, ld=None):
        rows = self.n if rows is None else rows
        need = L.clipmi_tempscale_workspace_bytes(rows)
        self.ws, self.theta, self.out = _ws(need, 2 * rows, misalign), _f32(torch.tensor([theta])), Guarded(2, F32)
        self.order = None if order is None else _Order(order)
        rc = L.clipmi_tempscale_batch(self.cos.ptr, self.ld if ld is None else ld, self.y.ptr, None if order is None else self.order.ptr, rows, self.n,
                                      self.C, self.theta.ptr, self.out.ptr, self.ws.ptr + misalign, need - short, _stream())
        torch.cuda.synchronize()
        return rc

    def fit(self, theta, order, batch, epochs, lrs, momentum=0.0, wd=0.0, drop_last=0):
        need = L.clipmi_tempscale_workspace_bytes(min(batch, self.n))
        self.ws, self.lr, self.loss = _ws(need, 2 * min(batch, self.n)), _f32(torch.tensor(lrs)), Guarded(len(lrs), F32)
        self.state = _f32(torch.tensor([theta, 0.0, 0.0, 0.0]))
        self.order = None if order is None else _Order(order)
        rc = L.clipmi_tempscale_fit(self.cos.ptr, self.ld, self.y.ptr, None if order is None else self.order.ptr, self.n, self.C, batch, epochs,
                                    drop_last, self.lr.ptr, momentum, 0.0, wd, 0, self.state.ptr, self.loss.ptr, self.ws.ptr, need, _stream())
        torch.cuda.synchronize()
        return rc

    def values(self, what, names):
        for g, n in ((self.cos, "cosine"), (self.ws, "workspace of exactly the reported bytes")):
            g.result(f"{what}: {n}")
        return {n: getattr(self, n).result(f"{what}: {n}") for n in names}


# (shape, ld - C)
TEMPSCALE_CASES = [((5, 65), 0), ((257, 1000), 8), ((1025, 3), 0)]


@pytest.mark.parametrize("case", TEMPSCALE_CASES, ids=str)
def test_tempscale_batch_and_step_within_bound(case):
    shape, ld_extra = case
    k = ref.tempscale_case(shape)
    bound = ref.tempscale_bound(shape)
    pairs = []
    for via_order in (False, True):
        for _ in range(2):
            perm = _perm(shape[0])[0] if via_order else None
            t = TempScale(k["c"], k["y"], ld_extra, perm)
            _lib.check(t.batch(ref.THETA, perm), f"tempscale {case}")
            pairs.append(t.values(f"tempscale {case}", ("out", "theta"))["out"])
        _assert_bits(pairs[-1], pairs[-2], "tempscale batch: two launches on the same input differ")
        _note("tempscale", "pair", case + (("order",) if via_order else ()), pairs[-1], bound["pair"])
    _assert_bits(pairs[0], pairs[2], "a row's pair does not depend on where the row lies: with and without a row list")
    states = []
    for _ in range(2):
        t = TempScale(k["c"], k["y"], ld_extra)
        _lib.check(t.fit(ref.THETA, None, shape[0], 1, [ref.TEMP_LR], momentum=0.9), f"tempscale fit {case}")
        states.append(t.values(f"tempscale fit {case}", ("state", "loss")))
    _same(states[0], states[1], f"tempscale fit {case}")
    st, loss = states[0]["state"], states[0]["loss"]
    _note("tempscale", "theta", case, st[0:1], bound["theta"])
    _assert_bits(st[1:2], pairs[0][1:2], "the momentum buffer of a first step is the batch gradient")
    _assert_bits(st[3:4], pairs[0][0:1], "state[3] is the batch loss")
    _assert_bits(loss, pairs[0][0:1], "the loss history is the batch loss")
    assert int(st.view(torch.int32)[2]) == 1
    th = F(ref.THETA)
    _assert_bits(st[0:1], _t32(F(th - F(F(ref.TEMP_LR) * pairs[0][1].numpy()))), "theta' == fl(theta - fl(lr g))")


def test_tempscale_ragged_fit_equals_batches():
    """n = 257 at 1000 classes in batches of 100 for two epochs through `order` (a last step of 57 rows in a workspace sized for 100): every
    step's loss has the bits clipmi_tempscale_batch returns on the same rows at the same theta, and theta follows torch.optim.SGD's rule in
    fp32 on those gradients bit for bit."""
    k = ref.tempscale_case(BIG_TEMPSCALE)
    n = BIG_TEMPSCALE[0]
    order = _perm(n, seed=9, epochs=2)
    mom, wd = F(0.9), F(5e-4)
    fit = TempScale(k["c"], k["y"], 8)
    _lib.check(fit.fit(ref.THETA, order, 100, 2, RAGGED_RATES, momentum=float(mom), wd=float(wd)), "tempscale ragged fit")
    want = fit.values("tempscale ragged fit", ("state", "loss"))
    th, buf = F(ref.THETA), F(0)
    one = TempScale(k["c"], k["y"], 8)
    for step, (e, j) in enumerate((e, j) for e in range(2) for j in range(3)):
        idx = order[e, 100 * j:100 * j + 100]
        _lib.check(one.batch(float(th), idx, rows=len(idx)), f"tempscale batch {step}")
        out = one.values(f"tempscale batch {step}", ("out",))["out"].numpy()
        _assert_bits(_t32(out[0]), want["loss"][step:step + 1], f"tempscale: batch vs fit: loss {step}")
        g = F(out[1] + F(wd * th))
        buf = g if step == 0 else F(F(mom * buf) + F(F(1.0) * g))
        th = F(th - F(F(RAGGED_RATES[step]) * buf))
    _assert_bits(want["state"][0:2], _t32(th, buf), "tempscale: batches vs fit: theta and the momentum buffer")
    assert int(want["state"].view(torch.int32)[2]) == 6 and np.isfinite(th) and th != F(ref.THETA)


@pytest.mark.parametrize("kind", ["label=C", "label=-1", "order=n"])
def test_tempscale_bad_label_or_index_poisons_and_never_addresses(kind):
    k = ref.tempscale_case(BIG_TEMPSCALE)
    n, C = BIG_TEMPSCALE
    y, order = np.array(k["y"]), np.arange(n, dtype=np.int32)
    if kind == "order=n":
        order[130] = n
    else:
        y[130] = C if kind == "label=C" else -1
    t = TempScale(k["c"], y, 8)
    _lib.check(t.batch(ref.THETA, order if kind == "order=n" else None), f"tempscale {kind}")
    assert torch.isnan(t.values(f"tempscale {kind}", ("out",))["out"]).all()
    _lib.check(t.fit(ref.THETA, order, n, 1, [ref.TEMP_LR]), f"tempscale fit {kind}")
    v = t.values(f"tempscale fit {kind}", ("state", "loss"))
    assert torch.isnan(v["loss"]).all() and torch.isnan(v["state"][0]) and int(v["state"].view(torch.int32)[2]) == 1
    # one row per batch at rate 0, the bad sample last: a row's pair does not depend on its batch, every earlier loss keeps the clean bits
    last = np.concatenate([np.delete(np.arange(n, dtype=np.int32), 130), order[130:131]])
    clean = TempScale(k["c"], k["y"], 8)
    _lib.check(clean.fit(ref.THETA, np.concatenate([last[:-1], [130]]), 1, 1, [0.0] * n), f"tempscale {kind}: clean rows")
    want = clean.values(f"tempscale {kind}: clean rows", ("loss",))["loss"]
    _lib.check(t.fit(ref.THETA, last, 1, 1, [0.0] * n), f"tempscale {kind}: rows")
    v = t.values(f"tempscale {kind}: rows", ("state", "loss"))
    assert torch.isfinite(want).all()
    _assert_bits(v["loss"][:-1], want[:-1], f"tempscale {kind}: the rows before the bad one")
    assert torch.isnan(v["loss"][-1]) and torch.isnan(v["state"][0]) and int(v["state"].view(torch.int32)[2]) == n


def test_tempscale_rejections_write_nothing():
    k = ref.tempscale_case((5, 65))
    for kw, want in ((dict(short=1), _lib.ERR_WORKSPACE), (dict(misalign=4), _lib.ERR_ARG), (dict(ld=64), _lib.ERR_SHAPE)):
        t = TempScale(k["c"], k["y"])
        assert t.batch(ref.THETA, **kw) == want, kw
        assert t.out.untouched() and t.ws.untouched(), kw
        t.values(f"tempscale rejected {kw}", ())


def test_zz_report_ratios():
    """The device's largest |err| / bound per method, value and case."""
    for k in sorted(RATIOS):
        print(f"cached-fits-parity: worst {k[0]:>9s} {k[1]:>7s} {k[2]:>44s} {RATIOS[k]:.4f}")
    assert all(v <= 1.0 for v in RATIOS.values())
