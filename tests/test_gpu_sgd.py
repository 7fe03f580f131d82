"""-m gpu: HipSGD (csrc/optim.hip k_sgd: SGD with Nesterov momentum, coupled weight decay and a device-side warm-up of lr
and momentum) against a float64 torch.optim.SGD, step by step under a derived bound; bit-exact invariants (packet path
against an unaligned view, no warm-up, a clip that never engages, the EMA, a captured graph against eager steps); clipping,
both loss-scaling routes, the EMA shadows, the state-dict round trip through torch.optim.SGD; and the model level
(CapturedTraining in fp32 and fp16, deterministic mode, checkpoints).

The bound.  The kernel forms, each line one rounding (u = 2^-24), from fp32 coefficients rounded from doubles:
    gg = fl(g*gs);  d = fma(wd, p, gg);  buf' = fma(mu, buf, d);  n = fma(mu, buf', d);  p' = fma(-lr, n, p)
Against the float64 rule stepped from the SAME fp32 state, per element:
    E_d = u(|d| + |wd*p|)  (+ u|g*gs| when gs != 1)          result rounding + the rounding of wd
    E_b = u(|buf'| + |mu*buf|) + E_d
    E_n = u(|n| + |mu*buf'|) + mu*E_b + E_d                   (E_n = E_b without Nesterov)
    E_p = u_store*|p'| + lr*(E_n + u|n|)                      u_store = 2^-24 / 2^-9 / 2^-11 for an fp32 / bf16 / f16 parameter
The tests allow 2x: the project's usual headroom over a counted number of roundings."""

import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
NANO = dict(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256])

# every layout: a multiple of 4 over several chunks, sizes 1 and 3, a chunk edge (4096, 4097), a gradient that is a view one
# element into its storage (4-byte aligned only), an fp32 parameter with a bf16 `lowp_grad`, a bf16 parameter with an fp32
# gradient, a parameter without gradient: 36 276 elements
SHAPES = [(64, 32, 3, 3), (1,), (3,), (4096,), (4097,), (5000,), (4099,), (515,), (33,)]
VIEW, LOWP, BF16P, NOGRAD = 5, 6, 7, 8
STD = 0.004                     # norm ~ 0.76 * scale: scales 1 / 0.01 pass a clipping threshold of 1, 30 / 5 do not
SCALES = (1.0, 30.0, 0.01, 5.0)
U = 2.0 ** -24
HEADROOM = 2.0
LR, MU, WD = 0.02, 0.937, 5e-4


def _params(seed, bf16=True):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(*s, generator=g) for s in SHAPES]
    if bf16:
        ps[BF16P] = ps[BF16P].bfloat16()
    return [nn.Parameter(p.cuda()) for p in ps]


def _grad_values(seed, scale):
    """The gradient VALUES of one step as the kernel sees them (fp32 on the host; the LOWP one already rounded to bf16)."""
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(*s, generator=g) * (STD * scale) for s in SHAPES]
    vals[LOWP] = vals[LOWP].bfloat16().float()
    vals[NOGRAD] = None
    return vals


def _give(ps, vals):
    for i, (p, v) in enumerate(zip(ps, vals)):
        p.grad = p.lowp_grad = None
        if v is None:
            continue
        if i == VIEW:
            buf = torch.zeros(v.numel() + 1, device="cuda")
            buf[1:].copy_(v)
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4
        elif i == LOWP:
            p.lowp_grad = v.bfloat16().cuda()
        elif p.dtype != torch.float32:
            p.lowp_grad = v.cuda()          # torch refuses an fp32 .grad on a bf16 parameter; the optimizer reads this one
        else:
            p.grad = v.cuda()


def _schedule(t, lr, mu, W, mu0, s0):
    """(lr_t, mu_t) of step t = 1, 2, ... in Python doubles: the definition of the warm-up."""
    if W > 0 and t <= W:
        f = (t - 1) / W
        return lr * (s0 + (1.0 - s0) * f), mu0 + (mu - mu0) * f
    return lr, mu


def _u_store(p):
    return {torch.float32: U, torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}[p.dtype]


def _reference(p0, buf0, g, gs, lr, mu, wd, nesterov, u_store):
    """One step of a float64 torch.optim.SGD from the device's state (p0, buf0: the fp32 values as float64; buf0 None = the
    buffer is still unset) -> p', buf', E_p, E_b and the three mutants' p'."""
    q = nn.Parameter(p0.clone())
    opt = torch.optim.SGD([q], lr=lr, momentum=mu, dampening=0, weight_decay=wd, nesterov=nesterov)
    if buf0 is not None:
        opt.state[q]["momentum_buffer"] = buf0.clone()
    gg = g * gs
    q.grad = gg.clone()
    opt.step()
    p1 = q.detach()
    b0 = torch.zeros_like(p0) if buf0 is None else buf0
    d = wd * p0 + gg
    # momentum 0: torch neither keeps nor touches a buffer; the kernel's equals d (the documented deviation)
    buf1 = opt.state[q]["momentum_buffer"] if mu != 0.0 else d
    n = mu * buf1 + d if nesterov else buf1
    e_d = U * (d.abs() + (wd * p0).abs()) + (U * gg.abs() if gs != 1.0 else 0.0)
    e_b = U * (buf1.abs() + (mu * b0).abs()) + e_d
    e_n = U * (n.abs() + (mu * buf1).abs()) + mu * e_b + e_d if nesterov else e_b
    e_p = u_store * p1.abs() + lr * (e_n + U * n.abs())
    bd = mu * b0 + gg                       # decoupled weight decay
    bm = mu * b0 + (1.0 - mu) * d           # dampening = mu
    mutants = dict(heavy_ball=p0 - lr * buf1,
                   decoupled=p0 * (1.0 - lr * wd) - lr * (mu * bd + gg if nesterov else bd),
                   dampening=p0 - lr * (mu * bm + d if nesterov else bm))
    return p1, buf1, e_p, e_b, mutants


def _state64(opt, ps):
    """(p, buf or None) of every parameter as float64 on the host"""
    out = []
    for p in ps:
        b = opt.state[p].get("momentum_buffer") if p in opt.state else None
        out.append((p.detach().double().cpu(), None if b is None else b.double().cpu()))
    return out


def _check_step(opt, ps, before, vals, gs, lr_t, mu_t, wd, nesterov, tag, mutant_frac=None):
    """Every stepped parameter's p and buf inside HEADROOM * (E_p, E_b); -> worst error / bound as text (fp32 parameters,
    the bf16 parameter, buffers).  `mutant_frac`: a dict that collects, per mutant, the fraction of the fp32 elements it
    leaves outside HEADROOM * E_p on this step."""
    after = _state64(opt, ps)
    worst_p = worst_l = worst_b = 0.0
    out, total = {}, 0
    for i, (p, v) in enumerate(zip(ps, vals)):
        if v is None:
            assert torch.equal(after[i][0], before[i][0]), (tag, i)
            continue
        p1, buf1, e_p, e_b, mutants = _reference(before[i][0], before[i][1], v.double(), gs, lr_t, mu_t, wd, nesterov, _u_store(p))
        err_p, err_b = (after[i][0] - p1).abs(), (after[i][1] - buf1).abs()
        if p.dtype == torch.float32:
            worst_p = max(worst_p, float((err_p / e_p.clamp_min(1e-300)).max()))
        else:
            worst_l = max(worst_l, float((err_p / e_p.clamp_min(1e-300)).max()))
        worst_b = max(worst_b, float((err_b / e_b.clamp_min(1e-300)).max()))
        assert bool((err_p <= HEADROOM * e_p).all()), (tag, "param", i, float((err_p / e_p.clamp_min(1e-300)).max()))
        assert bool((err_b <= HEADROOM * e_b).all()), (tag, "buf", i, float((err_b / e_b.clamp_min(1e-300)).max()))
        if mutant_frac is not None and p.dtype == torch.float32:
            total += p.numel()
            for name, pm in mutants.items():
                out[name] = out.get(name, 0) + int(((after[i][0] - pm).abs() > HEADROOM * e_p).sum())
    if mutant_frac is not None:
        for name, k in out.items():
            mutant_frac.setdefault(name, []).append(k / total)
    return f"worst error / E_p {worst_p:.3f} (fp32) {worst_l:.3f} (bf16)  / E_b {worst_b:.3f}"


def _parity_run(steps, nesterov, mu, warmup, lr_change=None, seed=0, mutants=False, tag="sgd"):
    from src.training.fused_sgd import HipSGD
    a = _params(seed)
    W, mu0, s0 = warmup
    oa = HipSGD(a, lr=LR, momentum=mu, weight_decay=WD, nesterov=nesterov, warmup_steps=W, warmup_momentum=mu0, warmup_lr_scale=s0)
    lr = LR
    fracs = {} if mutants else None
    for s in range(steps):
        if lr_change is not None and s + 1 == lr_change[0]:
            lr = oa.param_groups[0]["lr"] = lr_change[1]
        vals = _grad_values(1000 * seed + 100 + s, SCALES[s % 4])
        before = _state64(oa, a)
        if s == 0:
            assert all(b is None for _, b in before)            # step 1 starts from an unset buffer on both sides
        _give(a, vals)
        oa.step()
        lr_t, mu_t = _schedule(s + 1, lr, mu, W, mu0, s0)
        worst = _check_step(oa, a, before, vals, 1.0, lr_t, mu_t, WD, nesterov, (tag, s + 1), fracs)
        print(f"\n[{tag}] step {s + 1}: lr_t {lr_t:.6g} mu_t {mu_t:.6g}  {worst}", end="")
        assert float(oa.state[a[0]]["step"]) == s + 1
    return oa, a, fracs


def test_per_step_parity_with_float64_torch_sgd_and_the_mutants_leave_the_bound():
    """12 steps, Nesterov, wd 5e-4, warm-up over 5 steps from 0.1 * lr and momentum 0.8, lr change at step 8.  The power
    check: heavy-ball, decoupled weight decay and dampening = mu, stepped in float64 from the same state, each leave
    2 * E_p on more than half of the fp32 elements on at least one step."""
    oa, a, fracs = _parity_run(12, True, MU, (5, 0.8, 0.1), lr_change=(8, 0.005), mutants=True, tag="sgd nesterov")
    assert oa.state[a[0]]["momentum_buffer"].dtype == torch.float32 and oa.state[a[BF16P]]["momentum_buffer"].dtype == torch.float32
    assert set(fracs) == {"heavy_ball", "decoupled", "dampening"}
    for name, f in fracs.items():
        print(f"\n[sgd mutants] {name}: outside 2 E_p on {max(f):.4f} of the fp32 elements at its best step", end="")
        assert max(f) > 0.5, (name, f)


@pytest.mark.parametrize("nesterov,mu", [(False, MU), (False, 0.0)], ids=["heavy_ball", "momentum_0"])
def test_per_step_parity_without_nesterov_and_without_momentum(nesterov, mu):
    oa, a, _ = _parity_run(4, nesterov, mu, (0, 0.8, 0.0), seed=1, tag=f"sgd nesterov={nesterov} mu={mu}")
    if mu == 0.0:                           # the documented deviation: the buffer is kept, and it is d
        assert all(oa.state[p]["momentum_buffer"].abs().max() > 0 for i, p in enumerate(a) if i != NOGRAD)


# ------------------------------------------------------------------------------------------------ bit-exact invariants
def _same(oa, a, ob, b, tag=""):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (tag, "param", i)
        if i != NOGRAD:
            assert torch.equal(oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"]), (tag, "buf", i)


def test_packet_path_and_an_unaligned_view_give_the_same_bits():
    from src.training.fused_sgd import HipSGD
    g = torch.Generator().manual_seed(7)
    n = 2 * 4096 + 8                                            # a multiple of 4 over three chunks
    w0 = torch.randn(n, generator=g)
    store = torch.zeros(n + 1, device="cuda")
    store[1:].copy_(w0)
    a, b = nn.Parameter(w0.cuda()), nn.Parameter(store[1:])
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4
    kw = dict(lr=LR, momentum=MU, weight_decay=WD, warmup_steps=2, ema_decay=0.9, ema_tau=3.0)
    oa, ob = HipSGD([a], **kw), HipSGD([b], **kw)
    for s in range(3):
        v = (torch.randn(n, generator=g) * 0.01).cuda()
        a.grad, b.grad = v, v.clone()
        oa.step(), ob.step()
        assert torch.equal(a, b), s
        assert torch.equal(oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"]), s
        assert torch.equal(oa.ema_shadow(a), ob.ema_shadow(b)), s
    assert not torch.equal(a.detach().cpu(), w0)


def test_no_warmup_an_idle_clip_and_the_ema_leave_the_update_bits_alone():
    from src.training.fused_sgd import HipSGD
    kw = dict(lr=LR, momentum=MU, weight_decay=WD)
    ps = [_params(2) for _ in range(4)]
    opts = [HipSGD(ps[0], **kw), HipSGD(ps[1], warmup_steps=0, warmup_momentum=0.5, warmup_lr_scale=0.3, **kw),
            HipSGD(ps[2], max_grad_norm=1e30, **kw), HipSGD(ps[3], ema_decay=0.9, ema_tau=3.0, **kw)]
    for s in range(4):
        vals = _grad_values(300 + s, SCALES[s])
        for p, o in zip(ps, opts):
            _give(p, vals)
            o.step()
        assert float(opts[2].last_clip_coef) == 1.0
    for k in (1, 2, 3):
        _same(opts[0], ps[0], opts[k], ps[k], k)
    assert not torch.equal(opts[3].ema_shadow(ps[3][0]), ps[3][0].detach())


def test_replays_of_a_captured_step_equal_eager_steps_with_lr_and_warmup_changes_between_replays():
    """One eager warm-up step, the capture, six replays on regenerated gradients; the lr changes before replay 2 and
    warmup_steps before replay 1, both through sync_hyper() without recapture.  The twin takes eager steps on the same
    gradient values."""
    from src.training.fused_sgd import HipSGD
    a, b = _params(5), _params(5)
    kw = dict(lr=LR, momentum=MU, weight_decay=WD, warmup_steps=4, warmup_lr_scale=0.1, max_grad_norm=1.0, ema_decay=0.9, ema_tau=3.0)
    oa, ob = HipSGD(a, **kw), HipSGD(b, **kw)
    static = [torch.zeros(*s, device="cuda") for s in SHAPES]

    def produce(ps):                        # fresh gradient tensors every time (like autograd), values from `static`
        for i, (p, s) in enumerate(zip(ps, static)):
            p.grad = p.lowp_grad = None
            if i == NOGRAD:
                continue
            if i == VIEW:
                buf = torch.zeros(s.numel() + 1, device="cuda")
                buf[1:].copy_(s)
                p.grad = buf[1:]
            elif i == LOWP:
                p.lowp_grad = s.bfloat16()
            elif p.dtype != torch.float32:
                p.lowp_grad = s * 1.0
            else:
                p.grad = s * 1.0

    gen = torch.Generator(device="cuda").manual_seed(6)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s_ in static:
            s_.normal_(generator=gen).mul_(STD)
        produce(a), produce(b)
        oa.step(), ob.step()                # eager warm-up step (allocates tables, state, clip buffers and shadows)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same(oa, a, ob, b, "warm-up")
    for p in a:
        p.grad = p.lowp_grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        produce(a)
        oa.step()
    oa.finish_capture()
    for r in range(6):
        if r == 1:
            oa.warmup_steps = ob.warmup_steps = 6
        if r == 2:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 0.005
        oa.sync_hyper()
        for s_ in static:
            s_.normal_(generator=gen).mul_(STD * SCALES[r % 4])
        g.replay()
        produce(b)
        ob.step()
        _same(oa, a, ob, b, r)
        assert torch.equal(oa.last_clip_coef, ob.last_clip_coef)
        assert all(torch.equal(oa.ema_shadow(x), ob.ema_shadow(y)) for i, (x, y) in enumerate(zip(a, b)) if i != NOGRAD)
    torch.cuda.synchronize()
    assert float(oa.state[a[0]]["step"]) == 7 == float(ob.state[b[0]]["step"])


# ------------------------------------------------------------------------------------------------ clip, loss scaling, EMA
def test_clipped_steps_follow_clip_grad_norm_then_float64_sgd():
    """The gradient term of the reference is scaled by the device's own last_clip_coef (its accuracy against
    clip_grad_norm_'s is held by test_gpu_grad_clip.py; here it is compared at that test's 4e-6 as a plausibility check)."""
    from src.training.fused_sgd import HipSGD
    a = _params(3)
    oa = HipSGD(a, lr=LR, momentum=MU, weight_decay=WD, warmup_steps=3, warmup_lr_scale=0.1, max_grad_norm=1.0)
    clipped = []
    for s in range(6):
        vals = _grad_values(400 + s, SCALES[s % 4])
        before = _state64(oa, a)
        _give(a, vals)
        kept = [None if p.grad is None else p.grad.clone() for p in a]
        oa.step()
        twin = [nn.Parameter(torch.zeros(v.shape, dtype=torch.float64)) for v in vals if v is not None]
        for q, v in zip(twin, [v for v in vals if v is not None]):
            q.grad = v.double().clone()
        norm = float(torch.nn.utils.clip_grad_norm_(twin, 1.0))
        coef = float(oa.last_clip_coef)
        want = min(1.0, 1.0 / (norm + 1e-6))
        assert abs(coef - want) <= 4e-6 * want and ((coef < 1.0) == (norm > 1.0)), (s, coef, want)
        clipped.append(coef < 1.0)
        lr_t, mu_t = _schedule(s + 1, LR, MU, 3, 0.8, 0.1)
        worst = _check_step(oa, a, before, vals, coef, lr_t, mu_t, WD, True, ("clip", s + 1))
        print(f"\n[sgd clip] step {s + 1}: norm {norm:.6g} coef {coef:.6g}  {worst}", end="")
        assert all(k is None or torch.equal(k, p.grad) for k, p in zip(kept, a))        # the gradients are left alone
    assert clipped == [False, True, False, True, False, True]


@pytest.mark.parametrize("route", ["device_scaler", "gradscaler_protocol"])
def test_an_overflow_skips_everything_and_the_next_step_is_the_unscaled_update(route):
    """finite, inf, finite, nan, finite, finite with growth_interval 2.  A skipped step leaves p, buf, shadows, `step` and
    `ema_updates` untouched and halves the scale; the warm-up continues from the unadvanced t."""
    from src.training.fused_adamw import DeviceGradScaler
    from src.training.fused_sgd import HipSGD
    a = _params(4)
    W, mu0, s0 = 4, 0.8, 0.1
    oa = HipSGD(a, lr=LR, momentum=MU, weight_decay=WD, warmup_steps=W, warmup_momentum=mu0, warmup_lr_scale=s0,
                ema_decay=0.9, ema_tau=3.0)
    oa.ema_prepare()
    if route == "device_scaler":
        mine = oa.device_amp = DeviceGradScaler("cuda", init_scale=4096.0, growth_interval=2)
    else:
        mine = torch.amp.GradScaler("cuda", init_scale=4096.0, growth_interval=2)
        mine.scale(torch.zeros(1, device="cuda"))
    poison = {1: float("inf"), 3: float("nan")}
    t, scales = 0, []
    for s in range(6):
        sc = mine.get_scale()
        scales.append(sc)
        vals = [None if v is None else v * sc for v in _grad_values(500 + s, SCALES[s % 4])]     # sc: a power of two
        vals[LOWP] = vals[LOWP].bfloat16().float()
        if s in poison:
            vals[2][1] = poison[s]
        before = _state64(oa, a)
        shadows = [oa.ema_shadow(p).clone() for p in a]
        _give(a, vals)
        if route == "device_scaler":
            oa.step()
        else:
            mine.step(oa)
            mine.update()
        if s in poison:
            after = _state64(oa, a)
            for i in range(len(a)):
                assert torch.equal(after[i][0], before[i][0]), (s, i)
                assert (after[i][1] is None and before[i][1] is None) or torch.equal(after[i][1], before[i][1]), (s, i)
                assert torch.equal(oa.ema_shadow(a[i]), shadows[i]), (s, i)
            assert mine.get_scale() == 0.5 * sc
            if route == "device_scaler":
                assert mine.last_step_skipped()
        else:
            t += 1
            lr_t, mu_t = _schedule(t, LR, MU, W, mu0, s0)
            worst = _check_step(oa, a, before, vals, 1.0 / sc, lr_t, mu_t, WD, True, (route, s))
            print(f"\n[sgd amp {route}] step {s}: scale {sc} t {t}  {worst}", end="")
            assert any(not torch.equal(oa.ema_shadow(p), e) for p, e in zip(a, shadows))
        assert float(oa.state[a[0]]["step"]) == t == float(oa.ema_updates)
    assert t == 4 and scales == [4096.0, 4096.0, 2048.0, 2048.0, 1024.0, 1024.0] and mine.get_scale() == 2048.0


def test_shadows_follow_the_float64_recurrence_over_the_stored_weights():
    """tests/test_gpu_ema.py's bound for the same tail: after T updates |e_dev - e_64| <= T * 2^-23 * max(|e_0|, max_t |w_t|),
    w_t the parameter as stored (a bf16 parameter's rounded value), df and omd rounded to fp32 from the float64 d_t."""
    import math
    from src.training.fused_sgd import HipSGD
    decay, tau = 0.9, 3.0
    a = _params(6)
    oa = HipSGD(a, lr=LR, momentum=MU, weight_decay=WD, warmup_steps=3, warmup_lr_scale=0.1, ema_decay=decay, ema_tau=tau)
    oa.ema_prepare()
    e64 = [p.detach().double() for p in a]
    mx = [e.abs() for e in e64]
    assert all(torch.equal(oa.ema_shadow(p), p.detach().float()) for p in a)
    for s in range(6):
        _give(a, _grad_values(600 + s, SCALES[s % 4]))
        oa.step()
        d = decay * (1.0 - math.exp(-(s + 1) / tau))
        df = float(torch.tensor(d, dtype=torch.float64).float())
        omd = float(torch.tensor(1.0 - d, dtype=torch.float64).float())
        worst = 0.0
        for i, p in enumerate(a):
            if i == NOGRAD:
                continue
            w = p.detach().double()
            e64[i] = df * e64[i] + omd * w
            mx[i] = torch.maximum(mx[i], w.abs())
            bound = (s + 1) * 2.0 ** -23 * mx[i]
            err = (oa.ema_shadow(p).double() - e64[i]).abs()
            assert bool((err <= bound).all()), (s, i, float(err.max()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        print(f"\n[sgd ema] update {s + 1}: worst error / bound {worst:.3f}", end="")
        assert float(oa.ema_updates) == s + 1
    assert torch.equal(oa.ema_shadow(a[NOGRAD]), a[NOGRAD].detach())
    lag = max(float((oa.ema_shadow(p) - p.detach().float()).abs().max()) for i, p in enumerate(a) if i != NOGRAD)
    assert lag > 100 * 6 * 2.0 ** -23 * 4, lag                  # the average really lags: the bound is not vacuous


def test_state_dict_round_trip_through_torch_sgd_continues_bit_identically():
    """fp32 parameters: torch's load_state_dict casts state tensors to the parameter's dtype, which would round a bf16
    parameter's fp32 buffer (as it does HipAdamW's moments)."""
    from src.training.fused_sgd import HipSGD
    kw = dict(lr=LR, momentum=MU, weight_decay=WD, warmup_steps=6, warmup_lr_scale=0.1)
    a = _params(8, bf16=False)
    oa = HipSGD(a, **kw)
    for s in range(3):
        _give(a, _grad_values(800 + s, SCALES[s % 4]))
        oa.step()
    mid = [nn.Parameter(p.detach().clone()) for p in a]
    ot = torch.optim.SGD(mid, lr=1.0)
    ot.load_state_dict(copy.deepcopy(oa.state_dict()))       # load_state_dict keeps the tensors it is given: copy, as a file would
    assert ot.param_groups[0]["lr"] == LR and ot.param_groups[0]["nesterov"] is True and ot.param_groups[0]["momentum"] == MU
    assert torch.equal(ot.state[mid[0]]["momentum_buffer"], oa.state[a[0]]["momentum_buffer"])
    b = [nn.Parameter(p.detach().clone()) for p in a]
    ob = HipSGD(b, lr=1.0, momentum=0.5, nesterov=False, warmup_steps=6, warmup_lr_scale=0.1)
    ob.load_state_dict(copy.deepcopy(ot.state_dict()))
    assert ob.param_groups[0]["capturable"] is True and ob.param_groups[0]["momentum"] == MU
    for s in range(3, 6):
        vals = _grad_values(800 + s, SCALES[s % 4])
        _give(a, vals), _give(b, vals)
        oa.step(), ob.step()
        _same(oa, a, ob, b, s)
    assert float(ob.state[b[0]]["step"]) == 6 == float(oa.state[a[0]]["step"])        # the warm-up position survived
    # a torch.optim.SGD state (no `step`; a buffer torch never set) loads too: step 0, zeros
    c = [nn.Parameter(p.detach().clone()) for p in a]
    oc = torch.optim.SGD(c, lr=LR, momentum=MU, nesterov=True, weight_decay=WD)
    vals = _grad_values(860, 1.0)
    for q, v in zip(c, vals):
        q.grad = None if v is None else v.cuda()
    oc.step()
    d = [nn.Parameter(p.detach().clone()) for p in c]
    od = HipSGD(d, lr=LR, momentum=MU, weight_decay=WD)
    od.load_state_dict(copy.deepcopy(oc.state_dict()))
    _give(d, _grad_values(861, 1.0))
    od.step()
    assert float(od.state[d[0]]["step"]) == 1
    assert int(torch.count_nonzero(od.state[d[NOGRAD]]["momentum_buffer"])) == 0
    assert all(float(od.state[q]["momentum_buffer"].abs().max()) > 0 for i, q in enumerate(d) if i != NOGRAD)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_a_state_loaded_into_an_optimizer_that_has_already_stepped_is_the_one_that_is_stepped(kind):
    """load_state_dict replaces the state tensors the job table points at; the next step must rebuild the table (both
    optimizers share that code).  Three steps, a checkpoint, two more steps; then the checkpoint goes back into the SAME
    optimizer and the same two steps must end at the same bits, parameters and state."""
    from src.training.fused_adamw import HipAdamW
    from src.training.fused_sgd import HipSGD
    a = _params(9, bf16=False)
    if kind == "sgd":
        oa, names = HipSGD(a, lr=LR, momentum=MU, weight_decay=WD, warmup_steps=6, warmup_lr_scale=0.1), ("momentum_buffer",)
    else:
        oa, names = HipAdamW(a, lr=1e-3, weight_decay=1e-2), ("exp_avg", "exp_avg_sq")

    def steps(lo, hi):
        for s in range(lo, hi):
            _give(a, _grad_values(900 + s, SCALES[s % 4]))
            oa.step()
        return [p.detach().clone() for p in a] + [oa.state[p][k].clone() for p in a for k in names] + \
            [oa.state[a[0]]["step"].clone()]

    steps(0, 3)
    saved_p, saved_sd = [p.detach().clone() for p in a], copy.deepcopy(oa.state_dict())
    want = steps(3, 5)
    with torch.no_grad():
        for p, q in zip(a, saved_p):
            p.copy_(q)
    oa.load_state_dict(saved_sd)
    got = steps(3, 5)
    assert float(got[-1]) == 5
    bad = [i for i, (x, y) in enumerate(zip(want, got)) if not torch.equal(x, y)]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ model level
def _batch(seed=21):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(2, 3, 160, 160, generator=g).cuda()
    gts = [torch.cat([torch.rand(c, 2, generator=g) * 160, torch.rand(c, 2, generator=g) * 60 + 8,
                      torch.randint(0, 80, (c, 1), generator=g).float()], 1) for c in (3, 5)]
    return img, gts


@pytest.mark.parametrize("precision", ["float32", "float16"])
def test_captured_training_accepts_hipsgd(precision):
    """train()'s captured route: the first call steps eagerly and captures, then 8 replays on one fixed batch.  The lr is
    small on purpose: the loss of two 160 x 160 images is not smooth in the weights (the assignment of anchors to boxes is
    discrete), and at lr 1e-4 it fell from 4.11 to 3.70 over the nine steps but rose again by up to 0.3 on single steps."""
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training.fused_adamw import DeviceGradScaler
    from src.training.fused_sgd import HipSGD
    from src.training.train_model import CapturedTraining
    img, gts = _batch()
    torch.manual_seed(0)
    model = Model(**NANO, num_classes=80).cuda().train()
    opt = HipSGD(model.parameters(), lr=1e-5, momentum=0.9, weight_decay=5e-4, warmup_steps=3, warmup_lr_scale=0.1,
                 max_grad_norm=10.0)
    ct = CapturedTraining(model, YoloDFLQFLoss(num_classes=80), opt, precision)
    assert ct.usable
    first = ct.step(img, gts)["total_loss"]
    assert ct.captured and ct.runner.graph is not None and ct.runner.opt_in_graph
    assert (precision == "float16") == isinstance(getattr(opt, "device_amp", None), DeviceGradScaler)
    losses = [ct.step(img, gts)["total_loss"] for _ in range(8)]
    torch.cuda.synchronize()
    print(f"\n[sgd model {precision}] first {first:.5f} then {' '.join(f'{x:.5f}' for x in losses)}; "
          f"steps taken {float(opt.state[next(iter(opt.state))]['step']):.0f}", end="")
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    # Every buffer is non-zero whenever the kernel had anything to write: d = wd*p + g, so whenever the parameter or its
    # last gradient has a non-zero element.  What is left is named and must be what it can only be: a zero-initialised bias
    # of a box branch of the head that no positive anchor reached on this batch (its gradient is exactly zero, it stays 0).
    trainable = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert all(p.grad is not None for _, p in trainable)
    idle = [n for n, p in trainable if not bool(p.detach().any()) and not bool(p.grad.any())]
    print(f"\n[sgd model {precision}] zero parameter and zero gradient: {idle}", end="")
    assert all(n.startswith("head.box.") and n.endswith("bias") for n in idle), idle
    for n, p in trainable:
        assert (n in idle) != (float(opt.state[p]["momentum_buffer"].abs().max()) > 0.0), n
    assert losses[-1] < first, (first, losses)


def test_deterministic_mode_two_captured_runs_are_bit_identical():
    """The configuration of test_gpu_train_loop.py's deterministic test (bf16, capture + three replays), with HipSGD."""
    from src.hipops import functions as F_
    from src.model.losses import PackedTargets, YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training.fused_sgd import HipSGD
    from src.training.graph_step import TrainStepRunner
    img, gts = _batch(31)
    gts = [t.cuda() for t in gts]

    def run():
        torch.manual_seed(0)
        model = Model(**NANO, num_classes=80).cuda().train()
        opt = HipSGD(model.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4, warmup_steps=3, ema_decay=0.9, ema_tau=3.0)
        r = TrainStepRunner(model, YoloDFLQFLoss(num_classes=80), opt, "bfloat16", use_graph=True)
        r.capture(img, PackedTargets(gts, img.device), warmup=1)
        for _ in range(3):
            r.step()
        torch.cuda.synchronize()
        assert r.graph is not None and r.opt_in_graph
        ps = [p for p in model.parameters() if p.requires_grad]
        return [p.detach().clone() for p in ps] + [opt.state[p]["momentum_buffer"].clone() for p in ps] + \
            [opt.ema_shadow(p).clone() for p in ps] + [r.scalars.clone()]

    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert F_.deterministic_stats()
        a, b = run(), run()
    finally:
        torch.use_deterministic_algorithms(False)
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]
    assert not bad, (len(bad), len(a))


def test_checkpoint_round_trip_resumes_with_equal_bits(tmp_path):
    from src.model.model_builder import Model
    from src.training.ema import ModelEMA
    from src.training.fused_sgd import HipSGD
    from src.training.utils_train import load_checkpoint, save_checkpoint

    def make():
        model = Model(**NANO, num_classes=80).cuda().train()
        opt = HipSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4, warmup_steps=6, warmup_lr_scale=0.1)
        return model, opt, ModelEMA(model, opt, decay=0.9, tau=3.0)

    def synthetic_step(model, opt, seed):   # the same gradients on both sides
        g = torch.Generator(device="cuda").manual_seed(seed)
        with torch.no_grad():
            for p in model.parameters():
                if p.requires_grad:
                    p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3
            for b in model.buffers():
                if b.is_floating_point():
                    b.add_(torch.randn(b.shape, generator=g, device="cuda") * 1e-3)
        opt.step()

    def tensors(model, opt, ema):
        ps = [p for p in model.parameters() if p.requires_grad]
        return [p.detach() for p in ps] + [opt.state[p]["momentum_buffer"] for p in ps] + \
            [opt.ema_shadow(p) for p in ps] + list(ema._buf_shadows)

    torch.manual_seed(1)
    a = make()
    for s in range(3):
        synthetic_step(a[0], a[1], 900 + s)
    save_checkpoint(a[0], a[1], 1, 0.0, checkpoint_dir=str(tmp_path), ema=a[2])
    torch.manual_seed(2)
    b = make()
    assert load_checkpoint(b[0], b[1], str(tmp_path / "model_epoch_1.pth"), map_location="cuda", ema=b[2]) == 1
    assert b[2].updates == 3
    synthetic_step(a[0], a[1], 950), synthetic_step(b[0], b[1], 950)
    assert float(b[1].state[next(iter(b[0].parameters()))]["step"]) == 4        # the warm-up went on from step 3
    assert all(torch.equal(x, y) for x, y in zip(tensors(*a), tensors(*b)))
    assert b[2].updates == 4
