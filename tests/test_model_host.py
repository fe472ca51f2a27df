"""CPU tier of the composed model (tests/_model_ref.py): the float64 twin that tests/test_model_gpu.py holds the device to is itself held
to central differences, its dropout mask to the Philox definition, its inputs to the conditions that make them harder than the N(0, 0.1) of
the operator tests, and its optimizer step to tests/_optimize_ref.py."""
import numpy as np
import pytest

import _ewops_ref as ER
import _lstm_ref as LR
import _model_ref as M
import _optimize_ref as OR

NAMES = list(M.VARIANTS)


@pytest.fixture(scope="module", params=NAMES)
def case(request):
    twin = M.Twin(request.param)
    f = twin.forward()
    return twin, f, twin.backward(f)


def _fd(twin, key, direction, eps):
    base = np.asarray(twin.p[key], dtype=np.float64)
    up = twin.forward(values={key: base + eps * direction})["loss"]
    down = twin.forward(values={key: base - eps * direction})["loss"]
    return (up - down) / (2.0 * eps)


@pytest.mark.parametrize("key", M.PARAMS + M.EXTRA)
def test_analytic_gradient_matches_central_differences(case, key):
    """Every parameter, the gate, c0 and h0, in float64 with the dropout mask fixed: the derivative along a random direction over the
    whole tensor, and three single elements.  Central differences at eps = 1e-5 are good to eps^2 |f'''| + 1e-16 / eps, about 1e-10
    absolute; the bar is 1e-6 relative to the gradient's largest element times the direction's norm.  For Wx and the gate the derivative is the twin's
    ``*_true`` entry; what the operator registers instead is pinned by the test below."""
    twin, f, d = case
    grad = np.asarray(d[{"Wx": "Wx_true", "gx": "gx_true"}.get(key, key)], dtype=np.float64)
    assert grad.shape == twin.p[key].shape and np.abs(grad).max() > 0
    rng = np.random.RandomState(len(key) + grad.size)
    direction = rng.standard_normal(grad.shape)
    probes = [direction]
    for at in rng.permutation(np.flatnonzero(grad))[:3]:
        e = np.zeros(grad.size)
        e[at] = 1.0
        probes.append(e.reshape(grad.shape))
    for probe in probes:
        want, got = _fd(twin, key, probe, 1e-5), float((grad * probe).sum())
        assert abs(got - want) <= 1e-6 * np.abs(grad).max() * np.linalg.norm(probe) + 1e-12, (key, got, want)


def test_registered_gate_gradients(case):
    """dw_gated and gate_grad together: the registered weight gradient is the derivative times the gate once more, and dg is the gate
    times the derivative -- so both vanish on a block whose gate is 0 (the derivative of the gate does not)."""
    twin, f, d = case
    g = np.asarray(twin.p["gx"], dtype=np.float64)
    # (float64 sums over the time steps taken in another order: 1e-12 of the largest element covers an element that cancelled)
    assert np.allclose(d["Wx"], d["Wx_true"] * g[:, None, None], rtol=1e-12, atol=1e-12 * np.abs(d["Wx"]).max())
    assert np.allclose(d["gx"], d["gx_true"] * g, rtol=1e-12, atol=1e-12 * np.abs(d["gx"]).max())
    off = g == 0
    assert off.any() and not d["Wx"][off].any() and not d["Wx_true"][off].any() and not d["gx"][off].any() and d["gx_true"][off].all()


def test_mask_is_the_generating_calls(case):
    twin, f, d = case
    s = twin.spec
    words = ER.mask_words(M.N * s.H, M.SEED, M.OFFSET, M.KEEP)
    assert np.array_equal(twin.mask_words, words)
    assert np.array_equal(ER.unpack(words, M.N * s.H).reshape(twin.kept.shape), twin.kept)
    for i in (0, 1, 7, 8, M.N * s.H - 1):
        assert bool(twin.kept.reshape(-1)[i]) == bool(ER.keep_bit_loop(i, M.SEED, M.OFFSET, ER.threshold_of(M.KEEP)))
    later = M.Twin(s.name, step=2)
    assert np.array_equal(later.mask_words, ER.mask_words(M.N * s.H, M.SEED, M.OFFSET + 2, M.KEEP)) and not np.array_equal(later.mask_words, words)
    dropped = 1.0 - twin.kept.mean()
    assert 0.10 <= dropped <= 0.30, dropped
    assert np.array_equal(f["u"][~twin.kept], f["y"][~twin.kept])                   # a dropped element is its residual alone


def test_input_conditions(case):
    twin, f, d = case
    s = twin.spec
    ax = M.ax_of(s)
    zi, zu, zf, zo = LR._pre(f["c_in%d" % (M.T - 1)], LR.split(f["z%d" % (M.T - 1)], ax), twin.p["bg"], M.FB, ax)[1]
    sig = LR.sigmoid(np.concatenate([zi.reshape(-1), zf.reshape(-1), zo.reshape(-1)]))
    saturated = float(((sig < 0.02) | (sig > 0.98)).mean())
    assert 0.05 <= saturated <= 0.50, saturated
    counts = np.bincount(twin.tokens.reshape(-1), minlength=M.V)
    assert (counts == 0).sum() == 2 and not counts[list(M.ABSENT_ROWS)].any()
    assert counts.max() >= twin.tokens.size / 4.0 and counts.argmax() == M.HEAVY_ROW
    live = twin.labels[twin.labels >= 0]
    assert (twin.labels == -1).sum() == 1 and live.size == M.N - 1 and live.max() < s.classes
    # N - 1 live rows cannot name more than N - 1 classes: every class but two where the variant has at most N of them, else as many as
    # the rows allow with one class named twice
    assert np.unique(live).size == min(s.classes - 2, M.N - 2)
    g = twin.p["gx"]
    assert 0.15 <= (g == 0).mean() <= 0.25 and 0.15 <= (g == 1).mean() <= 0.25 and ((g != 0) & (g != 1)).any()
    assert f["loss_rows"][twin.labels < 0] == 0 and not d["rows"][twin.labels < 0].any()
    lay = M.layouts(s.name)
    assert all(min(l.shape) > 1 for l in lay.values())                              # more than one block each way


def test_optimizer_step_is_the_reference(case):
    """The twin's step calls _optimize_ref and nothing else: its results equal the helpers applied by hand, the first clip scales the
    gradients by CLIP_SHARE, gated-off blocks keep their values and a second step moves the moments on."""
    twin, f, d = case
    s = twin.spec
    clip = twin.clip_norm(d)
    state0 = twin.fresh_state()
    state1, (norm, scale) = twin.optimizer_step(state0, d, clip, 1)
    assert abs(scale - M.CLIP_SHARE) < 1e-12 and abs(norm - clip / M.CLIP_SHARE) < 1e-12 * norm
    lr_t = M.LRATE * OR.lr_correction_loop(1, 0.9, 0.999)
    for k in M.PARAMS:
        gate, bs = (twin.p["gx"], s.bsize) if k == "Wx" else (None, 0)
        p, m, v = OR.adam(state0[k][0], state0[k][1], state0[k][2], d[k], lr_t, gate=gate, bsize=bs, clip_sigma=M.CLIP_SIGMAS, norm_scale=scale)
        assert all(np.array_equal(a, b) for a, b in zip(state1[k][:3], (p, m, v))), k
        assert np.array_equal(state1[k][3], OR.ema(p, p, M.DECAY, gate, bs)) and np.array_equal(state1[k][3], p)
        assert not np.array_equal(p, state0[k][0])
    off = np.repeat(twin.p["gx"] == 0, s.bsize * s.bsize)
    for a, b in zip(state1["Wx"], state0["Wx"][:3] + (state0["Wx"][0],)):
        assert np.array_equal(a[off], b[off])
    state2, _ = twin.optimizer_step(state1, d, clip, 2)
    assert not np.array_equal(state2["bg"][3], state2["bg"][0]) and not np.array_equal(state2["bg"][1], state1["bg"][1])
    skipped, (_, zero) = twin.optimizer_step(state1, dict(d, bg=np.full_like(d["bg"], np.inf)), clip, 2)
    assert zero == 0.0 and all(np.array_equal(skipped[k][i], state1[k][i]) for k in M.PARAMS for i in range(3))


def test_float32_twin_is_close(case):
    """The float32 evaluation of the twin (the yardstick of the end-to-end GPU test) differs from float64 by float32 noise, not by a term."""
    twin, f, d = case
    f32 = twin.forward(prec="f32")
    d32 = twin.backward(f32)
    assert abs(f32["loss"] - f["loss"]) <= 1e-5 * abs(f["loss"])
    for k in M.PARAMS + M.EXTRA:
        err = np.linalg.norm(np.asarray(d32[k], dtype=np.float64) - d[k]) / np.linalg.norm(d[k])
        assert 0 < err <= 1e-4, (k, err)
