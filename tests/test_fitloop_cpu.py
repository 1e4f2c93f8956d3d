"""fitloop's two epoch loops, its order and schedule checks, driven on the CPU by a stepper that records what it is given."""
import math

import numpy as np
import pytest
import torch

from clip_calibration_amd import fitloop, tempfit

N, BS, EPOCHS = 5, 2, 2
RATES = [0.3, 0.007]
FEATURES = torch.arange(N, dtype=torch.float32).reshape(N, 1) * 10.0     # row i holds 10 i: a batch's rows are read off its values
LABELS = torch.tensor([2, 0, 1, 2, 1])


class Recorder:
    """Records (rows, labels, float(lr), want_loss) per step and returns the step's number as its loss."""

    def __init__(self):
        self.calls = []

    def __call__(self, f, y, lr, want_loss):
        assert lr.shape == (1,) and lr.dtype == torch.float32
        self.calls.append(((f[:, 0] / 10).long().tolist(), y.tolist(), float(lr), want_loss))
        return torch.tensor([float(len(self.calls) - 1)])


def run_cached(order, drop_last, return_history=True, epochs=EPOCHS):
    per_epoch = fitloop.steps_per_epoch(N, BS, drop_last)
    rates, lr_steps = fitloop.schedule("test", 0.0, epochs, RATES[:epochs], per_epoch, torch.device("cpu"))
    assert rates == RATES[:epochs]
    rec = Recorder()
    order_d = fitloop.order_on(fitloop.check_order("test", order, epochs, N), np.int64, torch.device("cpu"))
    hist = fitloop.run_cached(rec, FEATURES, LABELS, order_d, BS, per_epoch, epochs, lr_steps, return_history)
    return rec.calls, hist, per_epoch


@pytest.mark.parametrize("drop_last", [False, True])
def test_cached_loop_sequential(drop_last):
    calls, hist, per_epoch = run_cached(None, drop_last)
    want = [[0, 1], [2, 3]] + ([] if drop_last else [[4]])
    assert per_epoch == len(want) and [c[0] for c in calls] == want * EPOCHS
    assert [c[1] for c in calls] == [LABELS[r].tolist() for r in want] * EPOCHS
    assert all(c[3] is True for c in calls)
    for s, c in enumerate(calls):
        assert c[2] == float(np.float32(RATES[s // per_epoch]))
    assert hist.dtype == np.float32 and hist.tolist() == [float(s) for s in range(EPOCHS * per_epoch)]


@pytest.mark.parametrize("drop_last", [False, True])
def test_cached_loop_follows_order(drop_last):
    order = np.array([[3, 0, 4, 1, 2], [1, 4, 2, 0, 3]])
    calls, hist, per_epoch = run_cached(order, drop_last, return_history=False)
    assert hist is None and len(calls) == EPOCHS * per_epoch
    for s, (rows, labels, lr, want_loss) in enumerate(calls):
        e, k = divmod(s, per_epoch)
        assert rows == order[e, 2 * k:2 * k + 2].tolist() and labels == LABELS[order[e, 2 * k:2 * k + 2]].tolist()
        assert lr == float(np.float32(RATES[e])) and want_loss is False


def test_no_steps_give_an_empty_history():
    calls, hist, _ = run_cached(None, False, epochs=0)
    assert calls == [] and hist.dtype == np.float32 and hist.shape == (0,)
    _, lr_steps = fitloop.schedule("test", 0.1, 2, None, 0, torch.device("cpu"))
    ends = []
    hist = fitloop.run_batches(lambda *a: pytest.fail("no batch, no step"), [], 2, lr_steps, True, ends.append)
    assert hist.dtype == np.float32 and hist.shape == (0,) and ends == []
    assert fitloop.run_batches(lambda *a: None, [], 2, lr_steps, False) is None


def test_batch_loop_steps_and_epoch_ends():
    batches = ["a", "b", "c"]
    _, lr_steps = fitloop.schedule("test", 0.0, EPOCHS, RATES, len(batches), torch.device("cpu"))
    events = []

    def step(e, k, batch, lr, want_loss):
        events.append(("step", e, k, batch, float(lr), want_loss))
        return torch.tensor([float(len(events))])

    hist = fitloop.run_batches(step, batches, EPOCHS, lr_steps, True, lambda e: events.append(("end", e)))
    want = []
    for e in range(EPOCHS):
        want += [("step", e, k, b, float(np.float32(RATES[e])), True) for k, b in enumerate(batches)] + [("end", e)]
    assert events == want
    assert hist.tolist() == [float(i + 1) for i, ev in enumerate(events) if ev[0] == "step"]


class Loader:
    """A loader whose length says ``says`` and which gives ``gives`` batches."""

    def __init__(self, says, gives):
        self.says, self.gives = says, gives

    def __len__(self):
        return self.says

    def __iter__(self):
        return iter(range(self.gives))


def test_batch_loop_refuses_a_loader_that_miscounts():
    _, lr_steps = fitloop.schedule("test", 0.1, 1, None, 2, torch.device("cpu"))
    step = lambda e, k, b, lr, want: None
    with pytest.raises(RuntimeError, match="gave 1 batches in epoch 0, its length says 2"):
        fitloop.run_batches(step, Loader(2, 1), 1, lr_steps)
    with pytest.raises(RuntimeError, match="more than its length of 2 batches"):
        fitloop.run_batches(step, Loader(2, 3), 1, lr_steps)


def test_order_check():
    good = np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]])
    assert fitloop.check_order("who", None, EPOCHS, N) is None
    assert np.array_equal(fitloop.check_order("who", torch.from_numpy(good), EPOCHS, N), good)
    with pytest.raises(ValueError, match=r"who: order \(1, 5\) must be \[epochs, N\]"):
        fitloop.check_order("who", good[:1], EPOCHS, N)
    with pytest.raises(ValueError, match=r"who: order \(2, 4\) must be \[epochs, N\]"):
        fitloop.check_order("who", good[:, :4], EPOCHS, N)
    bad = good.copy()
    bad[1, 2] = N
    with pytest.raises(ValueError, match=r"who: order holds sample indices outside \[0, 5\)"):
        fitloop.check_order("who", bad, EPOCHS, N)
    bad[1, 2] = -1
    with pytest.raises(ValueError, match="outside"):
        fitloop.check_order("who", bad, EPOCHS, N)
    with pytest.raises(TypeError, match="who: order must be integers"):
        fitloop.check_order("who", good.astype(np.float32), EPOCHS, N)


def test_schedule():
    with pytest.raises(ValueError, match="who: 3 learning rates for 2 epochs"):
        fitloop.schedule("who", 0.1, 2, [0.1, 0.2, 0.3], 4, torch.device("cpu"))
    with pytest.raises(ValueError, match="who: 1 learning rates for 2 epochs"):
        fitloop.schedule("who", 0.1, 2, [0.1], 4, torch.device("cpu"))
    rates, lr_steps = fitloop.schedule("who", 0.002, 5, None, 3, torch.device("cpu"))
    assert rates == fitloop.cosine_warmup_schedule(0.002, 5)
    assert lr_steps.dtype == torch.float32 and lr_steps.tolist() == [float(np.float32(r)) for r in rates for _ in range(3)]
    # the docstring's formula: a constant warm-up epoch at 1e-5, then epoch e at lr (1 + cos(pi e / epochs)) / 2
    want = [1e-5] + [0.002 * (1.0 + math.cos(math.pi * e / 5)) / 2.0 for e in (1, 2, 3, 4)]
    assert fitloop.cosine_warmup_schedule(0.002, 5) == want
    assert tempfit.cosine_warmup_schedule is fitloop.cosine_warmup_schedule and tempfit.steps_per_epoch is fitloop.steps_per_epoch


def test_messages_name_the_function_called():
    """The shared checks speak under the caller's name; the SGD check refuses a weight decay that is not finite."""
    with pytest.raises(TypeError, match="fit_context: labels must be integers"):
        fitloop._labels("fit_context", np.array([0.0, 1.0]), 2, 3)
    with pytest.raises(ValueError, match=r"fit_context: labels span \[0, 3\]"):
        fitloop._labels("fit_context", [0, 3], 2, 3)
    for wd in (float("inf"), float("nan"), -1.0):
        with pytest.raises(ValueError, match="fit_adapter: weight_decay"):
            fitloop.check_sgd("fit_adapter", 0.9, 0.0, wd, False)
    with pytest.raises(ValueError, match="Nesterov"):
        fitloop.check_sgd("who", 0.0, 0.0, 0.0, True)
    with pytest.raises(ValueError, match="batch_size"):
        fitloop.check_run("who", 1, 0)
