"""sdc_critic_evaluate, sdc_value_loss and sdc_critic_backward on the device (include/sustaindc_hip.h THE CRITIC'S GRADIENT) against the
NumPy fp64 restatement (tests/critic_grad_ref.py).

1. critic_raw_values: critic_values of the same rows is raw * scale + shift in fp32, bit for bit -- rows 1, 15, 16, 17, 65, tanh and relu,
   with and without a ValueNorm; NaN rows behind the last row, poison behind the last value;
2. value_loss: loss and dvalue equal the restatement's rounding bit for bit (the arithmetic is + - * / and comparisons) at n = 1, 255,
   256, 257 and 37 x 40, all four flag combinations and the exact-tie inputs of tests/test_critic_grad_ref.py; stats redone bit for bit
   on the host from the stored outputs in the stated order;
3. critic_backward under the measure max|delta| / max|g| per parameter tensor, the worst tensor against the bar 8 x (torch fp32 CPU
   autograd's worst distance from the restatement on the same inputs: DESIGN.md section 4.28's bar, the reference arithmetic, not the
   code under test) at row counts around a tile, around a workgroup and SDC_CRITIC_GRAD_MAX_BLOCKS * 64 + 17 = 16 401 (one workgroup's
   second pass, the prefetch across it, a last tile of one row); NaN rows and NaN coefficients behind row R, poison behind element 6458;
   the rows come from a pool of 200 distinct rows per configuration whose relu pre-activations keep 1e-5 from zero (asserted);
4. bitwise: the same call twice, doubled coefficients, zero coefficients, grad_sq from the device's own grads, exact zeros for the
   feature LayerNorm when it is off, a relu network with b1 = -1000 whose w1, b1 and ln0 gradients are exactly zero;
5. the loop closed on collect(20) at 40 envs: critic_grads within the same bar, three SGD steps through assign_to and set_critic that
   lower the value loss at every step and stay within 8 x the distance a torch fp32 run of the same steps has from a torch fp64 run,
   the vector env's delegates, every refusal as ValueError with the library's text.
   Observed (DESIGN.md section 4.30 has the tables): the gradients 0.2 to 2.0 x torch fp32's distance, the dead relu layer with the
   feature LayerNorm on 6.3 x; the SGD steps' losses 6.6e-9 from torch fp64's, where torch fp32's are 1.85e-8 from them."""

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import actor_ref as AR
from tests import critic_grad_ref as GR
from tests import critic_ref as CR
from tests import onpolicy_ref as OR
from tests.plan_util import refused

pytestmark = pytest.mark.gpu

N = 40
MARGIN = 8.0
POOL = 200
LARGE = L.CRITIC_GRAD_MAX_BLOCKS * 64 + 17
COUNTS = [1, 15, 16, 17, 63, 64, 65, 67, LARGE]
POOL_SEED = {"tanh_fn1": 900, "tanh_fn0": 901, "relu_fn1": 902, "relu_fn0": 903}      # (relu: the margin below holds; checked on the CPU)
NAN32 = np.array([OR.NAN_BITS], dtype=np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def eng():
    e = AR.engine(N, False)
    yield e
    e.close()


def pool(activation, feature_norm):
    """200 distinct share_obs rows of the fixture's kind"""
    rng = np.random.default_rng(POOL_SEED[GR.cfg_name(activation, feature_norm)])
    x = rng.standard_normal((POOL, 29)).astype(np.float32)
    x[1::3, 20:] = 0.0
    return x


def inputs(activation, feature_norm, rows, seed):
    """rows of the pool (tiled past 200) with fresh coefficients: -> x [R, 29], dvalue [R]"""
    rng = np.random.default_rng(seed)
    x = pool(activation, feature_norm)[np.arange(rows) % POOL]
    coef = (rng.standard_normal(rows) / rows).astype(np.float32)
    coef[3::7] = 0.0
    return x, coef


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def padded_rows(e, x, extra=3):
    """the rows on the device with `extra` rows of NaN behind them"""
    import torch
    buf = np.full((x.shape[0] + extra, 29), NAN32, dtype=np.float32)
    buf[:x.shape[0]] = x
    return torch.from_numpy(buf).to(e.device)


def backward(e, x, coef, want_sq=True):
    """sdc_critic_backward of the rows, in buffers with three more rows of NaN rows and NaN coefficients behind row R, into grads with 7
    poisoned floats behind it -> (grads fp32 [6459], grad_sq float or None)"""
    import torch
    R, extra = x.shape[0], 3
    rows_d = padded_rows(e, x, extra)
    cf = np.full(R + extra, NAN32, dtype=np.float32)
    cf[:R] = coef
    cf_d = torch.from_numpy(cf).to(e.device)
    out = torch.full((L.CRITIC_N_PARAMS + 7,), OR.NAN_BITS, dtype=torch.int32, device=e.device).view(torch.float32)
    sq = torch.full((1,), -1.0, dtype=torch.float64, device=e.device) if want_sq else None
    e._behind_torch_stream()
    e._call(e.lib.sdc_critic_backward, rows_d.data_ptr(), R, cf_d.data_ptr(), out.data_ptr(), None if sq is None else sq.data_ptr(),
            e._stream(), refuses=True)
    got = out.cpu().numpy()
    assert (got[L.CRITIC_N_PARAMS:].view(np.uint32) == np.uint32(OR.NAN_BITS)).all()      # (the poison behind element 6458)
    g = got[:L.CRITIC_N_PARAMS].copy()
    assert np.isfinite(g).all(), R
    return g, (None if sq is None else float(sq.cpu()[0]))


def bar_of(sd, activation, x, coef, want):
    """torch fp32 CPU autograd's worst distance from the restatement `want` on these inputs"""
    import torch
    t32 = GR.torch_grads(GR.torch_net(sd, activation, torch.float32), x, coef)
    return max(GR.distance(t32, want).values())


# ---- 1. the raw values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value_norm", [None, CR.VALUE_NORM, (0.3, 1e-2)])
@pytest.mark.parametrize("activation,feature_norm", [("tanh", True), ("relu", False)])
def test_values_are_raw_times_scale_plus_shift_to_the_bit(eng, activation, feature_norm, value_norm):
    import torch
    c = GR.case(activation, feature_norm)
    eng.set_critic(c["sd"], value_norm, activation)
    scale, shift = np.float32(eng._critic.scale), np.float32(eng._critic.shift)
    for rows in (1, 15, 16, 17, 65):
        x, _ = inputs(activation, feature_norm, rows, 3)
        rows_d = padded_rows(eng, x)
        raw = torch.full((rows + 5,), OR.NAN_BITS, dtype=torch.int32, device=eng.device).view(torch.float32)
        eng._behind_torch_stream()
        eng._call(eng.lib.sdc_critic_evaluate, rows_d.data_ptr(), rows, raw.data_ptr(), eng._stream(), refuses=True)
        got = raw.cpu().numpy()
        assert (got[rows:].view(np.uint32) == np.uint32(OR.NAN_BITS)).all() and np.isfinite(got[:rows]).all()
        u = got[:rows]
        values = eng.critic_values(rows_d[:rows].contiguous()).cpu().numpy()
        assert np.array_equal(bits(values), bits(u * scale + shift)), (rows, value_norm)
        assert np.array_equal(bits(eng.critic_raw_values(rows_d[:rows].contiguous()).cpu().numpy()), bits(u))
        want = GR.backward(c["sd"], x, np.zeros(rows), activation)["u"]
        assert np.abs(u - want).max() <= 2e-4 * max(1.0, np.abs(want).max()), (rows, np.abs(u - want).max())      # (the critic's own bar)
    if value_norm is None:
        assert scale == 1.0 and shift == 0.0


# ---- 2. the value loss -----------------------------------------------------------------------------------------------------------------------
def _loss_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(shape).astype(np.float32)
    gap = np.where(rng.random(shape) < 0.5, rng.uniform(0.2, 0.6, shape), rng.uniform(0.0, 0.2, shape)) * rng.choice([-1.0, 1.0], shape)
    vp = (u + gap).astype(np.float32)
    vp.reshape(-1)[::9] = u.reshape(-1)[::9]
    ret = (40.0 + 12.0 * (u + 1.2 * rng.standard_normal(shape))).astype(np.float32)
    return u, vp, ret


def _check_value_loss(e, u, vp, ret, value_norm, clip, delta, flags, coef, want_loss=True):
    import torch
    from dc_rl_amd.engine import value_norm_scale_shift
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(e.device)
    res = e.value_loss(dev(u), dev(vp), dev(ret), clip, delta, bool(flags & 1), bool(flags & 2), value_norm=value_norm, coef=coef,
                       want_loss=want_loss)
    scale, shift = value_norm_scale_shift(value_norm)
    if value_norm is None and e._critic is not None:      # (None: the scale and shift of the critic in force)
        scale, shift = float(e._critic.scale), float(e._critic.shift)
    want = GR.value_loss(u, vp, ret, scale, shift, clip, delta, flags, 1.0 / u.size if coef is None else coef)
    dv = res.dvalue.cpu().numpy()
    assert dv.shape == u.shape and np.array_equal(bits(dv), bits(want["dvalue"])), (u.shape, flags)
    if want_loss:
        assert np.array_equal(bits(res.loss.cpu().numpy()), bits(want["loss"])), (u.shape, flags)
    else:
        assert res.loss is None
    st = res.stats.cpu().numpy()
    assert np.array_equal(st.view(np.uint64), GR.stats(want).view(np.uint64)), (u.shape, flags, st, GR.stats(want))
    assert res.summary() == GR.summary(st)
    return want, st


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_value_loss_is_the_restatement_to_the_bit(eng, flags):
    for shape in ((1,), (255,), (256,), (257,), (37, 40)):
        u, vp, ret = _loss_inputs(shape, 70 + shape[0])
        want, st = _check_value_loss(eng, u, vp, ret, (40.25, 11.5 ** 2), 0.2, 1.0, flags, None)
        if shape == (37, 40):
            assert (np.abs(want["eo"]) > 1.0).sum() > 100 and (np.abs(want["eo"]) <= 1.0).sum() > 100 and 100 < st[4] < 1380
            _check_value_loss(eng, u, vp, ret, (40.25, 11.5 ** 2), 0.2, 1.0, flags, 0.37, want_loss=False)
            _check_value_loss(eng, u, vp, ret, None, 0.0, 10.0, flags, -2.0)      # (clip 0: every d but 0 is outside)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_value_loss_at_every_tie_and_edge(eng, flags):
    from tests.test_critic_grad_ref import TIES
    u, vp, t = (np.array([c[i] for c in TIES], dtype=np.float32) for i in range(3))
    want, _ = _check_value_loss(eng, u, vp, t, (0.0, 1.0), 0.25, 1.0, flags, 0.5)
    assert want["d"][0] == 0.25 and want["lo"][7] == want["lc"][7] and want["eo"][10] == 0.0
    if flags & GR.CLIPPED:
        assert want["dvalue"][7] == np.float32(0.5 * 0.5 * 0.375) and want["dvalue"][11] == 0.0


def test_value_loss_defaults_to_the_critic_in_force(eng):
    import torch
    c = GR.case("tanh", True)
    eng.set_critic(c["sd"], CR.VALUE_NORM, "tanh")
    u, vp, ret = _loss_inputs((3, N), 5)
    dev = lambda a: torch.from_numpy(a).to(eng.device)
    a = eng.value_loss(dev(u), dev(vp), dev(ret))
    b = eng.value_loss(dev(u), dev(vp), dev(ret), value_norm=CR.VALUE_NORM, coef=1.0 / u.size)
    assert torch.equal(a.dvalue, b.dvalue) and torch.equal(a.loss, b.loss) and torch.equal(a.stats, b.stats)


# ---- 3. the gradients --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,feature_norm", GR.CONFIGS)
def test_gradients_against_the_restatement(eng, activation, feature_norm):
    c = GR.case(activation, feature_norm)
    name = GR.cfg_name(activation, feature_norm)
    eng.set_critic(c["sd"], CR.VALUE_NORM, activation)
    worst = (0.0, 0.0, None)
    for rows in COUNTS:
        x, coef = inputs(activation, feature_norm, rows, 40 + rows)
        want = GR.backward(c["sd"], x, coef, activation)
        if activation == "relu":
            assert GR.relu_margin(want) > 1e-5, (name, rows, GR.relu_margin(want))
        scale = bar_of(c["sd"], activation, x, coef, want)
        g, sq = backward(eng, x, coef)
        dist = GR.distance(GR.split(g), want)
        d = max(dist.values())
        print("%s %5d rows: device %.2e (%s), torch fp32 %.2e, ratio %.1f" % (name, rows, d, max(dist, key=dist.get), scale, d / scale))
        if worst[2] is None or d / scale > worst[0] / max(worst[1], 1e-300):
            worst = (d, scale, rows)
        assert d <= MARGIN * scale, (name, rows, dist, scale)
        assert sq == GR.grad_sq(g), (name, rows, sq, GR.grad_sq(g))
        if not feature_norm:
            assert not g[:58].any() and not np.signbit(g[:58]).any()      # (exact zeros)
    print("%s: worst device %.2e against torch fp32 %.2e at %d rows" % ((name,) + worst))


# ---- 4. bitwise ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,feature_norm,rows", [("tanh", True, 67), ("relu", False, 150), ("tanh", False, LARGE)])
def test_bitwise_properties(eng, activation, feature_norm, rows):
    c = GR.case(activation, feature_norm)
    eng.set_critic(c["sd"], None, activation)
    x, coef = inputs(activation, feature_norm, rows, 7)
    g, sq = backward(eng, x, coef)
    again, sq2 = backward(eng, x, coef)
    assert np.array_equal(bits(g), bits(again)) and sq == sq2                                     # the same call twice
    twice, sq4 = backward(eng, x, coef * np.float32(2.0))
    assert np.array_equal(bits(twice), bits(g * np.float32(2.0)))                                 # doubled exactly
    zero, sq0 = backward(eng, x, np.zeros_like(coef))
    assert not zero.any() and sq0 == 0.0                                                          # all-zero coefficients
    assert sq == GR.grad_sq(g) and sq4 == GR.grad_sq(twice)                                       # grad_sq from the device's own grads
    bare, none = backward(eng, x, coef, want_sq=False)
    assert none is None and np.array_equal(bits(g), bits(bare))
    if not feature_norm:
        assert not g[:58].any()
    # scale and shift are no parameters: the gradient does not see a ValueNorm
    eng.set_critic(c["sd"], CR.VALUE_NORM, activation)
    normed, _ = backward(eng, x, coef)
    assert np.array_equal(bits(g), bits(normed))


@pytest.mark.parametrize("feature_norm", [True, False])
def test_a_dead_relu_layer(eng, feature_norm):
    c = GR.case("relu", feature_norm)
    sd = {k: v.copy() for k, v in c["sd"].items()}
    sd[CR.KEYS["b1"]][:] = -1000.0
    eng.set_critic(sd, CR.VALUE_NORM, "relu")
    x, coef = inputs("relu", feature_norm, 67, 13)
    want = GR.backward(sd, x, coef, "relu")
    assert (want["z1"] < -100.0).all() and np.abs(want["z2"]).min() > 1e-5
    scale = bar_of(sd, "relu", x, coef, want)
    g, sq = backward(eng, x, coef)
    got = GR.split(g)
    for k in ("w1", "b1", "ln0_g", "ln0_b"):
        assert not got[k].any() and not want[k].any(), k
    d = max(GR.distance(got, want).values())
    print("dead relu layer fn%d: device %.2e, torch fp32 %.2e" % (feature_norm, d, scale))
    assert d <= MARGIN * scale and np.isfinite(g).all() and sq == GR.grad_sq(g)


# ---- 5. the loop closed --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def looped():
    """an engine with three tanh actors and a critic under a ValueNorm, and a batch of 20 steps collected with them"""
    e = AR.engine(N, False)
    nets = [AR.torch_actor(300 + a) for a in range(3)]
    AR.set_actors(e, nets)
    sd = CR.make_critic(21)
    e.set_critic(sd, CR.VALUE_NORM)
    e.reset()
    batch = e.collect(20)
    yield e, sd, batch
    e.close()


def _torch_step_losses(net, x, vp, ret, scale, shift, clip, delta, flags, lr, max_norm, steps):
    """the value loss before and after each of `steps` SGD steps (gradient clipped to max_norm as torch's clip_grad_norm_) in the
    module's dtype"""
    import torch
    dt = next(net.parameters()).dtype
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    xt, vpt, rt = (torch.as_tensor(a, dtype=dt) for a in (x, vp, ret))
    losses = []
    for step in range(steps + 1):
        opt.zero_grad()
        loss = GR.torch_value_loss(net(xt), vpt, rt, scale, shift, clip, delta, flags).mean()
        losses.append(float(loss.detach()))
        if step == steps:
            break
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm)
        opt.step()
    return losses


def test_critic_grads_close_the_loop(looped):
    import torch
    from dc_rl_amd.engine import value_norm_scale_shift
    from tests.test_gpu_actor_stats import _vec
    e, sd0, b = looped
    sd0 = {k: v.numpy() for k, v in sd0.items()}
    T, clip, delta, flags, lr, max_norm = b.n_steps, 0.2, 10.0, 3, 0.01, 1.0      # (lr 0.05 overshoots at the second step, in torch fp64 as well)
    scale, shift = value_norm_scale_shift(CR.VALUE_NORM)
    try:
        grads, terms = e.critic_grads(b, clip, delta)
        assert grads.flat.shape == (L.CRITIC_N_PARAMS,) and grads.sq_norm.dim() == 0 and terms.dvalue.shape == (T, N)
        # against the restatement fed the device's own raw values (the loss's branches are then the device's), then its own dvalue
        x = b.share_obs[:T].reshape(T * N, 29).cpu().numpy()
        vp, ret = b.value_preds[:T].reshape(-1).cpu().numpy(), b.returns.reshape(-1).cpu().numpy()
        raw = e.critic_raw_values(b.share_obs[:T])
        vl = GR.value_loss(raw.cpu().numpy().reshape(-1), vp, ret, scale, shift, clip, delta, flags, 1.0 / (T * N))
        dv = terms.dvalue.cpu().numpy().reshape(-1)
        assert np.array_equal(bits(dv), bits(vl["dvalue"])) and np.array_equal(bits(terms.loss.cpu().numpy().reshape(-1)), bits(vl["loss"]))
        assert np.array_equal(terms.stats.cpu().numpy().view(np.uint64), GR.stats(vl).view(np.uint64))
        want = GR.backward(sd0, x, dv, "tanh")
        bar = bar_of(sd0, "tanh", x, dv, want)
        g = grads.flat.cpu().numpy()
        d = max(GR.distance(GR.split(g), want).values())
        print("critic_grads on %d rows: device %.2e, torch fp32 %.2e; %s" % (T * N, d, bar, terms.summary()))
        assert d <= MARGIN * bar
        assert float(grads.sq_norm.cpu()) == GR.grad_sq(g) and abs(float(grads.norm().cpu()) - np.sqrt(GR.grad_sq(g))) <= 1e-15
        named = grads.named()
        assert list(named) == list(GR.FIELDS) and all(tuple(named[k].shape) == GR.SHAPES[k] for k in GR.FIELDS)
        mod = GR.torch_net(sd0, "tanh")
        assert set(grads.state_dict()) == set(mod.state_dict())
        assert all(tuple(v.shape) == tuple(mod.state_dict()[k].shape) for k, v in grads.state_dict().items())
        # value_loss_coef scales dvalue; the ValueNorm handed over is the one in force
        half, _ = e.critic_grads(b, clip, delta, value_loss_coef=0.5, value_norm=CR.VALUE_NORM)
        assert torch.equal(half.flat, grads.flat * 0.5)
        # the vector env's delegates return the same tensors
        v = _vec(N)
        try:
            v.reset()
            v.set_critic(sd0, CR.VALUE_NORM)
            dvc = v.engine.device
            share = b.share_obs[:T].contiguous().to(dvc)
            raw_v = v.critic_raw_values(share)
            assert torch.equal(raw_v.cpu(), raw.cpu())
            tv = v.value_loss(raw_v, b.value_preds[:T].contiguous().to(dvc), b.returns.to(dvc), clip, delta)
            assert torch.equal(tv.dvalue.cpu(), terms.dvalue.cpu()) and torch.equal(tv.stats.cpu(), terms.stats.cpu())
            theirs = v.critic_backward(share, tv.dvalue)
            assert torch.equal(theirs.flat.cpu(), grads.flat.cpu()) and torch.equal(theirs.sq_norm.cpu(), grads.sq_norm.cpu())
            assert dvc == e.device      # (both on device 0: the batch goes as it is)
            chained, tc = v.critic_grads(b, clip, delta)
            assert torch.equal(chained.flat, grads.flat) and torch.equal(tc.dvalue, terms.dvalue) and torch.equal(tc.loss, terms.loss)
        finally:
            v.close()
        # clip_: torch's clip_grad_norm_ rule
        before = grads.flat.clone()
        total = grads.clip_(0.5 * float(grads.norm()))
        assert float(total) == float(grads.norm()) and torch.allclose(grads.flat, before * 0.5, rtol=1e-5, atol=0.0)
        # three SGD steps through a plain torch module, assign_to and set_critic; torch fp32 and fp64 runs of the same steps beside them
        opt = torch.optim.SGD(mod.parameters(), lr=lr)
        losses = []
        for step in range(4):
            gr, tm = e.critic_grads(b, clip, delta)
            losses.append(tm.summary()["value_loss"])
            if step == 3:
                break
            gr.clip_(max_norm)
            gr.assign_to(mod)
            assert all(p.grad is not None and p.grad.shape == p.shape for p in mod.parameters())
            opt.step()
            e.set_critic(mod.state_dict(), CR.VALUE_NORM)
        run = lambda dt: _torch_step_losses(GR.torch_net(sd0, "tanh", dt), x, vp, ret, scale, shift, clip, delta, flags, lr, max_norm, 3)
        l32, l64 = run(torch.float32), run(torch.float64)
        gap = max(abs(a - c) for a, c in zip(losses, l64))
        gap32 = max(abs(a - c) for a, c in zip(l32, l64))
        print("value loss over three SGD steps: device %s, torch fp64 %s, gap %.2e; torch fp32's gap %.2e" % (losses, l64, gap, gap32))
        assert all(losses[i + 1] < losses[i] for i in range(3)), losses
        assert gap <= MARGIN * gap32, (gap, gap32)
    finally:
        e.set_critic(sd0, CR.VALUE_NORM)


def test_every_refusal_reaches_python_and_nothing_is_launched(looped):
    import torch
    e, sd, b = looped
    dev, T = e.device, 3
    share = torch.zeros((T, N, 29), device=dev)
    cf = torch.zeros((T, N), device=dev)
    poison = lambda n: torch.full((n,), OR.NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    out, raw, dvl, loss = poison(L.CRITIC_N_PARAMS), poison(T * N), poison(T * N), poison(T * N)
    sq = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    stats = torch.full((9,), -1.0, dtype=torch.float64, device=dev)
    p = lambda x: x.data_ptr()
    ev = lambda **kw: e._call(e.lib.sdc_critic_evaluate, kw.get("share", p(share)), kw.get("rows", T * N), kw.get("raw", p(raw)), e._stream(),
                              refuses=True)
    refused(e, "sdc_critic_evaluate: n_rows = 0 must be positive", lambda: ev(rows=0))
    refused(e, "sdc_critic_evaluate: null array", lambda: ev(raw=None))
    refused(e, "sdc_critic_evaluate: share_obs / raw_values not dword-aligned", lambda: ev(share=p(share) + 2))
    vl = lambda **kw: e._call(e.lib.sdc_value_loss, kw.get("n", T * N), kw.get("u", p(cf)), kw.get("vp", p(cf)), kw.get("ret", p(cf)),
                              kw.get("scale", 1.0), kw.get("shift", 0.0), kw.get("clip", 0.2), kw.get("delta", 10.0), kw.get("flags", 3),
                              kw.get("coef", 1.0), kw.get("loss", p(loss)), kw.get("dv", p(dvl)), kw.get("stats", p(stats)), e._stream(),
                              refuses=True)
    refused(e, "sdc_value_loss: n = 0 must be positive", lambda: vl(n=0))
    for name in ("u", "vp", "ret", "dv"):
        refused(e, "sdc_value_loss: null array \\(raw_values, value_preds, returns and dvalue are required\\)", lambda: vl(**{name: None}))
    refused(e, "sdc_value_loss: raw_values / value_preds / returns / loss / dvalue not dword-aligned", lambda: vl(loss=p(loss) + 1))
    refused(e, "sdc_value_loss: stats not 8-byte aligned", lambda: vl(stats=p(stats) + 4))
    refused(e, "sdc_value_loss: target_scale = 0.000000 must be finite and positive", lambda: vl(scale=0.0))
    refused(e, "sdc_value_loss: target_shift = inf is not finite", lambda: vl(shift=float("inf")))
    refused(e, "sdc_value_loss: flags = 4: unknown bits", lambda: vl(flags=4))
    refused(e, "sdc_value_loss: clip_param = -0.500000 must be finite and not negative", lambda: e.value_loss(cf, cf, cf, clip_param=-0.5))
    refused(e, "sdc_value_loss: huber_delta = 0.000000 must be finite and positive", lambda: e.value_loss(cf, cf, cf, huber_delta=0.0))
    for bad in (float("nan"), float("inf")):
        refused(e, "sdc_value_loss: coef = .* is not finite", lambda: e.value_loss(cf, cf, cf, coef=bad))
    bw = lambda **kw: e._call(e.lib.sdc_critic_backward, kw.get("share", p(share)), kw.get("rows", T * N), kw.get("cf", p(cf)),
                              kw.get("out", p(out)), kw.get("sq", p(sq)), e._stream(), refuses=True)
    refused(e, "sdc_critic_backward: n_rows = -1 must be positive", lambda: bw(rows=-1))
    for name in ("share", "cf", "out"):
        refused(e, "sdc_critic_backward: null array \\(share_obs, dvalue and grads are required\\)", lambda: bw(**{name: None}))
    refused(e, "sdc_critic_backward: share_obs / dvalue / grads not dword-aligned", lambda: bw(cf=p(cf) + 2))
    refused(e, "sdc_critic_backward: grad_sq not 8-byte aligned", lambda: bw(sq=p(sq) + 4))
    # the Python side's own checks, in its words
    refused(e, "critic_raw_values: share_obs must be a contiguous float32 CUDA tensor of shape \\(..., 29\\)", lambda: e.critic_raw_values(cf))
    refused(e, "critic_backward: share_obs must be a contiguous float32 CUDA tensor", lambda: e.critic_backward(share.cpu(), cf))
    refused(e, "critic_backward: dvalue must be", lambda: e.critic_backward(share, cf[:2]))
    refused(e, "value_loss: raw_values must be a contiguous float32 CUDA tensor", lambda: e.value_loss(cf.double(), cf, cf))
    refused(e, "value_loss: returns must be", lambda: e.value_loss(cf, cf, cf[:2]))
    refused(e, "value_loss: coef = 'x' must be a number", lambda: e.value_loss(cf, cf, cf, coef="x"))
    refused(e, "critic_params: value_norm must be None, a \\(mean, var\\) pair", lambda: e.value_loss(cf, cf, cf, value_norm=(1.0, 2.0, 3.0)))
    # before set_critic: the library's text
    fresh = AR.engine(N, False)
    try:
        with pytest.raises(ValueError, match="sdc_critic_backward: sdc_set_critic first"):
            fresh.critic_backward(share.to(fresh.device), cf.to(fresh.device))
        with pytest.raises(ValueError, match="sdc_critic_evaluate: sdc_set_critic first"):
            fresh.critic_raw_values(share.to(fresh.device))
        ok = fresh.value_loss(cf.to(fresh.device), cf.to(fresh.device), cf.to(fresh.device))      # (no critic needed: scale 1, shift 0)
        assert float(ok.stats.cpu()[7]) == T * N and not ok.dvalue.any()
    finally:
        fresh.close()
    torch.cuda.synchronize(dev)
    for x in (out, raw, dvl, loss):
        assert bool((x.view(torch.int32) == OR.NAN_BITS).all())
    assert float(sq[0]) == -1.0 and bool((stats == -1.0).all())
