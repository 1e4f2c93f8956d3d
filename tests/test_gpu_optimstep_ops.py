"""clipmi_block_step_adam and clipmi_block_step_adam_scaled (csrc/optim_step.hip) on the GPU against tests/optimstep_ref.py: the static
step bit for bit against the fp32 restatement in the kernel's order and within the criterion of torch's float64 Adam / AdamW; the scaled
step's bits against the static step's; an inf or a NaN at every seam of the 256-thread workgroups skips the step and the next clean step
takes the table row of the APPLIED count; the refusals of a call that could otherwise launch."""
import numpy as np
import pytest
import torch

import optimstep_ref as oref

pytestmark = pytest.mark.gpu

from clip_calibration_amd import _lib, fitloop, ops  # noqa: E402

RULES = [(False, 0.0), (False, 5e-4), (True, 0.0), (True, 5e-4)]
STEPS = 5
BIG = 10 ** 9      # a growth interval no test reaches


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def same(t, a):
    return np.array_equal(bits(t), np.asarray(a, np.float32).view(np.int32))


def table(steps=16, betas=oref.BETAS):
    return cuda(fitloop.adam_bias_table(betas, steps))


LR = torch.tensor([oref.LR], dtype=torch.float32)


@pytest.mark.parametrize("decoupled,wd", RULES)
@pytest.mark.parametrize("gs", [1.0, 4096.0])
@pytest.mark.parametrize("total", oref.SEAMS)
def test_static_step_equals_the_restatement_bit_for_bit(total, gs, decoupled, wd):
    assert oref.threads() == 256
    w0, g = oref.make_block(total, steps=STEPS)
    gsc = (g * np.float32(gs)).astype(np.float32)
    assert np.isfinite(gsc).all() and (g == 0).any() and (np.abs(g) == np.float32(1e4)).any()
    want = oref.emulate_run(w0, gsc, grad_scale=gs, weight_decay=wd, decoupled=decoupled)
    p, m, v, lr, tab = cuda(w0), torch.zeros(total).cuda(), torch.zeros(total).cuda(), LR.cuda(), table()
    got = []
    for k in range(STEPS):
        out = ops.block_step_adam(cuda(gsc[k]), p, m, v, lr, k + 1, tab, gs, weight_decay=wd, decoupled=decoupled)
        assert same(out, (gsc[k] * (np.float32(1.0) / np.float32(gs))).astype(np.float32)), k
        assert same(p, want[k][0]) and same(m, want[k][1]) and same(v, want[k][2]), k
        got.append(p.cpu().numpy().copy())
    t64 = oref.torch_run(w0, g, torch.float64, weight_decay=wd, decoupled=decoupled)
    t32 = oref.torch_run(w0, g, torch.float32, weight_decay=wd, decoupled=decoupled)
    err, bound = oref.within_torch(np.stack(got), t32, t64)
    print(f"optimstep: device total={total} gs={gs} decoupled={decoupled} wd={wd}: {err:.3e} <= {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("decoupled,wd", [(False, 5e-4), (True, 5e-4)])
@pytest.mark.parametrize("total", [257, 1000])
def test_scaled_step_with_finite_gradients_equals_the_static_step(total, decoupled, wd):
    w0, g = oref.make_block(total, steps=3)
    gs = 256.0
    gsc = (g * np.float32(gs)).astype(np.float32)
    lr, tab = LR.cuda(), table()
    ps, ms, vs = cuda(w0), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    pd, md, vd = cuda(w0), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    state = ops.new_scaler_state(gs, "cuda")
    for k in range(3):
        a = ops.block_step_adam(cuda(gsc[k]), ps, ms, vs, lr, k + 1, tab, gs, weight_decay=wd, decoupled=decoupled)
        b = ops.block_step_adam_scaled(cuda(gsc[k]), state, pd, md, vd, lr, tab, growth_interval=BIG, weight_decay=wd, decoupled=decoupled)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ps), bits(pd)) and np.array_equal(bits(ms), bits(md)) \
            and np.array_equal(bits(vs), bits(vd)), k
    assert ops.scaler_state_dict(state) == {"scale": gs, "growth_tracker": 3, "skipped_steps": 0, "applied_steps": 3, "found_inf": 0}
    assert not np.array_equal(bits(pd), w0.view(np.int32))


PLACES = [(256, 0), (256, 255), (257, 256)]     # the first element, the last of a full workgroup, the last of a partial last workgroup


@pytest.mark.parametrize("bad", [np.inf, np.nan])
@pytest.mark.parametrize("total,place", PLACES)
def test_a_non_finite_element_skips_the_step_and_the_table_row_is_the_applied_count(total, place, bad):
    w0, g = oref.make_block(total, steps=3)
    gs = 256.0
    rule = dict(weight_decay=5e-4, decoupled=False)
    lr, tab = LR.cuda(), table()
    p, m, v = cuda(w0), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    state = ops.new_scaler_state(gs, "cuda")
    ops.block_step_adam_scaled(cuda(g[0] * np.float32(gs)), state, p, m, v, lr, tab, growth_interval=BIG, **rule)
    before = [bits(t).copy() for t in (p, m, v)]
    poisoned = (g[1] * np.float32(gs)).astype(np.float32)
    poisoned[place] = bad
    ops.block_step_adam_scaled(cuda(poisoned), state, p, m, v, lr, tab, growth_interval=BIG, **rule)
    assert all(np.array_equal(bits(t), b) for t, b in zip((p, m, v), before))
    assert ops.scaler_state_dict(state) == {"scale": gs / 2, "growth_tracker": 0, "skipped_steps": 1, "applied_steps": 1, "found_inf": 1}
    ops.block_step_adam_scaled(cuda(g[2] * np.float32(gs / 2)), state, p, m, v, lr, tab, growth_interval=BIG, **rule)
    assert ops.scaler_state_dict(state) == {"scale": gs / 2, "growth_tracker": 1, "skipped_steps": 1, "applied_steps": 2, "found_inf": 0}
    # the static run of the two clean steps at the scales in force: the second one is Adam's step 2, not 3
    ps, ms, vs = cuda(w0), torch.zeros(total).cuda(), torch.zeros(total).cuda()
    ops.block_step_adam(cuda(g[0] * np.float32(gs)), ps, ms, vs, lr, 1, tab, gs, **rule)
    ops.block_step_adam(cuda(g[2] * np.float32(gs / 2)), ps, ms, vs, lr, 2, tab, gs / 2, **rule)
    assert np.array_equal(bits(p), bits(ps)) and np.array_equal(bits(m), bits(ms)) and np.array_equal(bits(v), bits(vs))
    want = oref.emulate_run(w0, g[[0, 2]], **rule)
    assert same(p, want[1][0])
    third = oref.emulate_run(want[0][0], g[2:3], t0=3, m=want[0][1], v=want[0][2], **rule)
    assert not same(p, third[0][0])             # the row of the step count would have given other bits


def test_refusals_leave_every_buffer_untouched():
    total = 300
    w0, g = oref.make_block(total, steps=1)
    p, m, v, lr = cuda(w0), torch.zeros(total).cuda(), torch.zeros(total).cuda(), LR.cuda()
    short = table(2)
    with pytest.raises(_lib.ClipmiError, match="t=3 lies behind the bias table of 2 steps"):
        ops.block_step_adam(cuda(g[0]), p, m, v, lr, 3, short)
    with pytest.raises(_lib.ClipmiError, match="t=0"):
        ops.block_step_adam(cuda(g[0]), p, m, v, lr, 0, short)
    with pytest.raises(_lib.ClipmiError, match="beta1"):
        ops.block_step_adam(cuda(g[0]), p, m, v, lr, 1, short, betas=(1.0, 0.999))
    with pytest.raises(_lib.ClipmiError, match="eps"):
        ops.block_step_adam(cuda(g[0]), p, m, v, lr, 1, short, eps=0.0)
    with pytest.raises(_lib.ClipmiError, match="weight_decay"):
        ops.block_step_adam(cuda(g[0]), p, m, v, lr, 1, short, weight_decay=-1.0)
    with pytest.raises(_lib.ClipmiError, match="grad_scale"):
        ops.block_step_adam(cuda(g[0]), p, m, v, lr, 1, short, 0.0)
    state = ops.new_scaler_state(16.0, "cuda")
    with pytest.raises(_lib.ClipmiError, match="growth_interval"):
        ops.block_step_adam_scaled(cuda(g[0]), state, p, m, v, lr, short, growth_interval=0)
    with pytest.raises(ValueError, match="same number of elements"):
        ops.block_step_adam(cuda(g[0][:10]), p, m, v, lr, 1, short)
    with pytest.raises(TypeError, match="exp_avg_sq"):
        ops.block_step_adam(cuda(g[0]), p, m, v[:10], lr, 1, short)
    with pytest.raises(TypeError, match="bias_table"):
        ops.block_step_adam(cuda(g[0]), p, m, v, lr, 1, short.float())
    with pytest.raises(TypeError, match="state"):
        ops.block_step_adam_scaled(cuda(g[0]), state[:4], p, m, v, lr, short)
    torch.cuda.synchronize()
    assert same(p, w0) and not m.any() and not v.any()
    assert ops.scaler_state_dict(state) == {"scale": 16.0, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 0, "found_inf": 0}
