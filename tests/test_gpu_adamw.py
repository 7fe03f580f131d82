"""-m gpu: HipAdamW's kernels (csrc/optim.hip k_adamw, k_grad_sqnorm, k_clip_finalize, k_found_inf, k_amp_update) under the
derived per-element bound of tests/strict_optim.py: every step against the float64 rule from the device's own state read back
before the step, at 2 x the bound, with six mutants that must leave it; the same under both loss-scaling routes and under
clipping; the bit-exact invariants that tests/test_gpu_sgd.py holds for SGD; a job table of 300 records with guard elements
around every tensor; and the small kernels called directly through the C ABI.  tests/test_gpu_optim.py and
tests/test_gpu_grad_clip.py pin a different property (nearness to torch's fp32 optimizer) and stay as they are."""
import math

import pytest
import torch
from torch import nn

import strict_optim as so
from test_gpu_grad_clip import NORM_RTOL

pytestmark = pytest.mark.gpu
U, HEADROOM = so.U, so.HEADROOM
SHAPES, KINDS = so.SHAPES, so.KINDS
IDX = {k: KINDS.index(k) for k in ("view", "g_bf16", "g_f16", "nograd", "p_bf16", "p_f16", "empty")}
LR, B1, B2, EPS, WD = so.HYPER
STORE = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "f16"}
YOLO_ERR_ARG = 1001


def _opt(ps, **kw):
    from src.training.fused_adamw import HipAdamW
    return HipAdamW(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, **kw)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(*s, generator=g).to(so.P_DTYPE.get(k, torch.float32)).cuda()) for s, k in zip(SHAPES, KINDS)]


def _stored(vals, sc=1.0):
    """The gradient VALUES as the kernel sees them: times the loss scale in fp32, a lowp_grad rounded to its 16-bit type."""
    out = []
    for v, k in zip(vals, KINDS):
        v = v * sc
        out.append(None if k == "nograd" else v.to(so.G_DTYPE[k]).float() if k in so.G_DTYPE else v)
    return out


def _give(ps, vals):
    for p, v, k in zip(ps, vals, KINDS):
        p.grad = p.lowp_grad = None
        if v is None:
            continue
        if k == "view":
            buf = torch.zeros(v.numel() + 1, device="cuda")
            buf[1:].copy_(v)
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4
        elif k in so.G_DTYPE:
            p.lowp_grad = v.to(so.G_DTYPE[k]).cuda()
        elif k in so.P_DTYPE:
            p.lowp_grad = v.cuda()          # torch refuses an fp32 .grad on a 16-bit parameter; the optimizer reads this one
        else:
            p.grad = v.cuda()


def _state64(opt, ps):
    """(p, exp_avg, exp_avg_sq) of every parameter as float64 on the host; moments that do not exist yet are zeros."""
    out = []
    for p in ps:
        st = opt.state[p] if p in opt.state else {}
        m, v = st.get("exp_avg"), st.get("exp_avg_sq")
        z = torch.zeros(p.shape, dtype=torch.float64)
        out.append((p.detach().double().cpu(), z if m is None else m.double().cpu(), z if v is None else v.double().cpu()))
    return out


def _check_step(opt, ps, before, vals, gs, hyper, t, tag, worst, fracs=None):
    """Every stepped tensor's p, exp_avg and exp_avg_sq inside HEADROOM * (E_p, E_m, E_v) of the float64 step from `before`;
    a parameter without gradient keeps its bits.  `fracs`: per mutant, (outside, of) on its block of the fp32 parameters."""
    after = _state64(opt, ps)
    out = {}
    for i, (p, v, k) in enumerate(zip(ps, vals, KINDS)):
        if v is None:
            assert all(torch.equal(a, b) for a, b in zip(after[i], before[i])), (tag, "no gradient", i)
            continue
        p0, m0, v0 = before[i]
        p1, m1, v1, e_p, e_m, e_v = so.adamw_ref(p0, v.double(), m0, v0, gs, hyper, t, p.dtype)
        for name, got, want, e in ((f"E_p[{STORE[p.dtype]}]", after[i][0], p1, e_p), ("E_m", after[i][1], m1, e_m),
                                   ("E_v", after[i][2], v1, e_v)):
            err = (got - want).abs()
            r = worst.add(name, err, e)
            assert bool((err <= HEADROOM * e).all()), (tag, name, i, k, r)
        if fracs is not None and p.dtype == torch.float32 and p.numel() >= 8:
            for name in so.MUTANTS:
                pm = so.adamw_ref(p0, v.double(), m0, v0, gs, hyper, t, p.dtype, name)[0]
                bad = ((after[i][0] - pm).abs() > HEADROOM * e_p).flatten()
                blk = so.eps_block(p.numel()) if name in so.EPS_BLOCK_MUTANTS else slice(None)
                a, b = out.get(name, (0, 0))
                out[name] = (a + int(bad[blk].sum()), b + bad[blk].numel())
    if fracs is not None:
        for name, (a, b) in out.items():
            fracs.setdefault(name, []).append(a / b)


def _report(tag, worst, fracs=None):
    print(f"\n[adamw {tag}] worst err / E (limit {HEADROOM:g}): {worst}", end="")
    for name, f in (fracs or {}).items():
        print(f"\n[adamw {tag}] mutant {name}: outside 2 E_p on {max(f):.4f} of its block at its best step", end="")


# ------------------------------------------------------------------------------------------------ 1, 2: per-step parity
def test_per_step_parity_with_the_float64_rule_and_every_mutant_leaves_the_bound():
    """8 steps, lr changed at step 5; lr 1e-2 and wd 0.1 make the place of the weight decay visible, the eps block the place
    of eps.  Each mutant, stepped in float64 from the same state, leaves 2 * E_p on more than half of its block of the fp32
    parameters on at least one step."""
    a = _params(0)
    oa = _opt(a)
    worst, fracs, lr = so.Worst(), {}, LR
    for s in range(8):
        if s + 1 == 5:
            lr = oa.param_groups[0]["lr"] = 2.5e-3
        vals = _stored(so.grad_values(SHAPES, 100 + s, s))
        before = _state64(oa, a)
        _give(a, vals)
        oa.step()
        _check_step(oa, a, before, vals, 1.0, (lr, B1, B2, EPS, WD), s + 1, ("parity", s + 1), worst, fracs)
        assert float(oa.state[a[0]]["step"]) == s + 1
    _report("parity", worst, fracs)
    assert int(torch.count_nonzero(oa.state[a[IDX["nograd"]]]["exp_avg"])) == 0      # the parameter without gradient: zeros still
    assert oa.state[a[IDX["p_bf16"]]]["exp_avg"].dtype == torch.float32 and a[IDX["p_f16"]].dtype == torch.float16
    assert set(fracs) == set(so.MUTANTS) and {"E_p[fp32]", "E_p[bf16]", "E_p[f16]", "E_m", "E_v"} <= set(worst.w)
    for name, f in fracs.items():
        assert max(f) > 0.5, (name, f)


@pytest.mark.parametrize("route", ["gradscaler_1024", "device_scaler_1536", "clip"])
def test_parity_under_loss_scaling_and_clipping(route):
    """gs of the reference is the fp32 value the kernel forms: 2^-10; fl(1 / 1536), which rounds; the device's own
    last_clip_coef (held against the float64 coefficient here at test_gpu_sgd.py's 4e-6, and by the finalize test below)."""
    from src.training.fused_adamw import DeviceGradScaler
    a = _params(1)
    oa = _opt(a, max_grad_norm=1.0 if route == "clip" else None)
    sc, scaler = 1.0, None
    if route == "gradscaler_1024":
        sc, scaler = 1024.0, torch.amp.GradScaler("cuda", init_scale=1024.0)
        scaler.scale(torch.zeros(1, device="cuda"))
    elif route == "device_scaler_1536":
        sc = 1536.0
        oa.device_amp = DeviceGradScaler("cuda", init_scale=sc)
    gs = float(torch.tensor(1.0) / torch.tensor(sc))            # the fp32 quotient, correctly rounded on both sides
    assert (gs * sc != 1.0) == (route == "device_scaler_1536")
    worst, clipped = so.Worst(), []
    for s in range(4):
        vals = _stored(so.grad_values(SHAPES, 200 + s, s), sc)
        before = _state64(oa, a)
        _give(a, vals)
        if scaler is not None:
            scaler.step(oa)
            scaler.update()
            assert scaler.get_scale() == sc
        else:
            oa.step()
        if route == "clip":
            gs = float(oa.last_clip_coef)
            sq = torch.stack([(v.double() ** 2).sum() for v in vals if v is not None])
            norm, want = so.clip_finalize_ref(sq, 1.0)
            assert abs(gs - want) <= 4e-6 * want and ((gs < 1.0) == (norm > 1.0)), (s, gs, want)
            clipped.append(gs < 1.0)
        _check_step(oa, a, before, vals, gs, so.HYPER, s + 1, (route, s + 1), worst)
        assert float(oa.state[a[0]]["step"]) == s + 1
    _report(route, worst)
    if route == "clip":
        assert clipped == [False, True, False, True]
    if route == "device_scaler_1536":
        assert oa.device_amp.get_scale() == sc and not oa.device_amp.last_step_skipped()


# ------------------------------------------------------------------------------------------------ 3: bit-exact invariants
def test_packet_path_and_an_unaligned_view_give_the_same_bits():
    g = torch.Generator().manual_seed(7)
    n = 2 * 4096 + 8                                            # a multiple of 4 over three chunks
    w0 = torch.randn(n, generator=g)
    store = torch.zeros(n + 1, device="cuda")
    store[1:].copy_(w0)
    a, b = nn.Parameter(w0.cuda()), nn.Parameter(store[1:])
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4
    oa, ob = _opt([a], ema_decay=0.9, ema_tau=3.0), _opt([b], ema_decay=0.9, ema_tau=3.0)
    for s in range(3):
        v = so.grad_values([(n,)], 300 + s, s)[0].cuda()
        a.grad, b.grad = v, v.clone()
        oa.step(), ob.step()
        assert torch.equal(a, b), s
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a][name], ob.state[b][name]), (s, name)
        assert torch.equal(oa.ema_shadow(a), ob.ema_shadow(b)), s
    assert not torch.equal(a.detach().cpu(), w0) and not torch.equal(oa.ema_shadow(a), a.detach())


def test_an_idle_clip_and_the_ema_leave_the_update_bits_alone():
    ps = [_params(2) for _ in range(3)]
    opts = [_opt(ps[0]), _opt(ps[1], max_grad_norm=1e30), _opt(ps[2], ema_decay=0.9, ema_tau=3.0)]
    for s in range(4):
        vals = _stored(so.grad_values(SHAPES, 400 + s, s))
        for p, o in zip(ps, opts):
            _give(p, vals)
            o.step()
        assert float(opts[1].last_clip_coef) == 1.0
    for k in (1, 2):
        for i, (x, y) in enumerate(zip(ps[0], ps[k])):
            assert torch.equal(x, y), (k, "param", i)
            if KINDS[i] != "nograd":
                for name in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(opts[0].state[x][name], opts[k].state[y][name]), (k, name, i)
    assert not torch.equal(opts[2].ema_shadow(ps[2][0]), ps[2][0].detach())


# ------------------------------------------------------------------------------------------------ 4: a job table of real size
def test_three_hundred_records_one_clipped_step_and_nothing_outside_a_tensor_moves():
    """300 parameters (the model has about 250), sizes cycling through a chunk edge and two chunks: 450 chunks, so
    k_clip_finalize's lanes take a second partial.  Parameters, gradients and both moments are views into four flat buffers
    with >= 4 pre-filled guard elements on both sides of every tensor; offsets are multiples of 4 elements, so sizes 4, 4096
    and 8192 take the packet path and the others the any-dtype path.  The moments start from values of a fifth step."""
    sizes = (1, 3, 4, 4095, 4096, 4097, 8192, 8193)
    N, T0 = 300, 5
    offs, off = [], 4
    for k in range(N):
        offs.append(off)
        off = (off + sizes[k % 8] + 4 + 3) // 4 * 4
    total = off
    g = torch.Generator().manual_seed(8)
    host = dict(p=torch.randn(total, generator=g), g=torch.full((total,), 5.0), m=torch.randn(total, generator=g) * 1e-3,
                v=(torch.randn(total, generator=g) * 3e-3) ** 2)
    inside = torch.zeros(total, dtype=torch.bool)
    grads = so.grad_values([(sizes[k % 8],) for k in range(N)], 500, 1)
    for k, o in enumerate(offs):
        inside[o:o + sizes[k % 8]] = True
        host["g"][o:o + sizes[k % 8]] = grads[k]
    for name, fill in (("p", 3.0), ("m", 7.0), ("v", 11.0)):
        host[name][~inside] = fill
    dev = {name: t.cuda() for name, t in host.items()}
    assert all(t.data_ptr() % 16 == 0 for t in dev.values())
    ps = [nn.Parameter(dev["p"][o:o + sizes[k % 8]]) for k, o in enumerate(offs)]
    assert ps[1].data_ptr() == dev["p"].data_ptr() + 4 * offs[1]
    oa = _opt(ps, max_grad_norm=1.0)
    for k, (p, o) in enumerate(zip(ps, offs)):
        n = sizes[k % 8]
        p.grad = dev["g"][o:o + n]
        oa.state[p] = dict(step=torch.tensor(float(T0)), exp_avg=dev["m"][o:o + n], exp_avg_sq=dev["v"][o:o + n])
    oa.step()
    assert oa._plans[0]["njobs"] == N and oa._plans[0]["nchunks"] == sum(-(-sizes[k % 8] // 4096) for k in range(N)) > 256
    assert float(oa.state[ps[0]]["step"]) == T0 + 1
    assert oa.state[ps[7]]["exp_avg"].data_ptr() == dev["m"].data_ptr() + 4 * offs[7]     # the views were adopted, not copied
    after = {name: t.cpu() for name, t in dev.items()}
    for name in ("p", "g", "m", "v"):
        assert torch.equal(after[name][~inside], host[name][~inside]), f"a guard element of {name} moved"
    assert torch.equal(after["g"], host["g"])
    want = math.sqrt(float((host["g"][inside].double() ** 2).sum()))
    got, coef = float(oa.last_grad_norm), float(oa.last_clip_coef)
    print(f"\n[adamw table] norm device {got:.9g} float64 {want:.9g} rel {abs(got - want) / want:.2e} coef {coef:.6g}", end="")
    assert abs(got - want) <= NORM_RTOL * want and coef < 0.5
    assert abs(coef - 1.0 / (want + 1e-6)) <= 4e-6 * coef
    d = {name: t.double() for name, t in host.items()}
    p1, m1, v1, e_p, e_m, e_v = so.adamw_ref(d["p"], d["g"], d["m"], d["v"], coef, so.HYPER, T0 + 1, torch.float32)
    worst = so.Worst()
    for name, key, ref, e in (("E_p[fp32]", "p", p1, e_p), ("E_m", "m", m1, e_m), ("E_v", "v", v1, e_v)):
        err = (after[key].double() - ref).abs()[inside]
        r = worst.add(name, err, e[inside])
        bad = (err > HEADROOM * e[inside]).nonzero().flatten()
        assert bad.numel() == 0, (name, r, inside.nonzero().flatten()[bad][:8].tolist())
    assert not torch.equal(after["p"][inside], host["p"][inside])
    _report("table", worst)


# ------------------------------------------------------------------------------------------------ 5 .. 8: the small kernels
def _job_table(records):
    """A device job table as HipFusedOptimizer._build builds it: records of (p, g, m, v) -> (jobs_dev, njobs, nchunks)."""
    from src.hipops import lib
    from src.hipops.ops import _p, dt
    jb = lib.query("yolo_adamw_job_bytes")
    host = torch.zeros(len(records) * jb, dtype=torch.uint8)
    for i, (p, g, m, v) in enumerate(records):
        assert g.numel() == p.numel() == m.numel() == v.numel() and g.is_contiguous()
        lib.call("yolo_adamw_job_fill", host.data_ptr(), i, _p(p), dt(p), _p(g), dt(g), _p(m), _p(v), p.numel())
    nchunks = lib.query("yolo_adamw_jobs_finalize", host.data_ptr(), len(records))
    return host.cuda(), len(records), nchunks


def test_grad_sqnorm_partials_per_chunk_on_both_routes():
    """Every partial inside 2 * 14 U * sum g^2 of its own chunk: the packet route (aligned fp32, a multiple of 4, with a last
    chunk of 8 elements), the scalar route with a bf16 and an f16 gradient, an odd length whose last chunk holds one element,
    and an unaligned view; an empty record's idle chunk gives 0."""
    from src.hipops import lib
    from src.hipops.ops import _p, _stream
    lens = [3 * 4096 + 8, 5000, 2 * 4096 + 1, 515, 4096, 0, 4097]
    kinds = ["packet", "bf16", "odd", "f16", "view", "empty", "chunk_edge"]
    vals = so.grad_values([(n,) for n in lens], 600, 1)
    gdev = []
    for v, k in zip(vals, kinds):
        if k == "view":
            buf = torch.zeros(v.numel() + 1, device="cuda")
            buf[1:].copy_(v)
            gdev.append(buf[1:])
        else:
            gdev.append(v.to({"bf16": torch.bfloat16, "f16": torch.float16}.get(k, torch.float32)).cuda())
    assert gdev[0].data_ptr() % 16 == 0 and gdev[4].data_ptr() % 16 == 4
    recs = [(torch.zeros(n, device="cuda"), g, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")) for n, g in zip(lens, gdev)]
    jobs, njobs, nchunks = _job_table(recs)
    assert nchunks == sum(max(1, -(-n // 4096)) for n in lens)
    partials = torch.full((nchunks + 2,), -1.0, device="cuda")
    found = torch.zeros(1, device="cuda")
    lib.call("yolo_grad_sqnorm", _p(jobs), njobs, nchunks, partials.data_ptr() + 4, _p(found), _stream(partials))
    got = partials.cpu().double()
    assert got[0] == -1.0 and got[-1] == -1.0 and float(found) == 0.0
    c, worst = 1, {}
    for n, g, k in zip(lens, gdev, kinds):
        gh = g.cpu()
        for lo in range(0, max(n, 1), 4096):
            want, e = so.sqnorm_ref(gh[lo:lo + 4096])
            err = abs(float(got[c]) - want)
            worst[k] = max(worst.get(k, 0.0), err / e if e else 0.0)
            assert err <= HEADROOM * e, (k, lo, float(got[c]), want, err / e if e else err)
            c += 1
    assert c == nchunks + 1
    print("\n[adamw sqnorm] worst err / (14 U sum g^2): " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()), end="")


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_clip_finalize_directly(n):
    """Hand-made partials; total_norm within 2 U (a float64 sum and root, one fp32 store) and coef within 4 U of float64,
    clipped and not, with and without a loss scale of 1536; an inf partial gives coef 0, a nan partial nan."""
    from src.hipops import lib
    from src.hipops.ops import _p, _stream
    g = torch.Generator().manual_seed(900 + n)
    parts = (torch.rand(max(n, 1), generator=g) * 2e-3 + 1e-7).cuda()        # a buffer even for n = 0: the entry refuses null
    scale = torch.tensor([1536.0], device="cuda")

    def run(p, max_norm, sc):
        state = torch.tensor([max_norm, -1.0, -1.0], device="cuda")
        lib.call("yolo_grad_clip_finalize", _p(p), n, _p(state), _p(sc), _stream(state))
        s = state.cpu()
        assert float(s[0]) == so.f32(max_norm)
        return float(s[1]), float(s[2])

    for sc in (None, scale):
        norm0, _ = so.clip_finalize_ref(parts[:n].cpu(), 1.0, None if sc is None else 1536.0)
        for max_norm in ((1.0,) if n == 0 else (so.f32(0.5 * norm0), so.f32(2.0 * norm0))):
            want_norm, want_coef = so.clip_finalize_ref(parts[:n].cpu(), max_norm, None if sc is None else 1536.0)
            norm, coef = run(parts, max_norm, sc)
            assert abs(norm - want_norm) <= 2 * U * want_norm, (n, norm, want_norm)
            assert abs(coef - want_coef) <= 4 * U * want_coef, (n, coef, want_coef)
            assert (coef == 1.0) == (want_coef == 1.0) and (n == 0) <= (norm == 0.0 and coef == 1.0)
    if n:
        for bad in (float("inf"), float("nan")):
            p = parts.clone()
            p[n - 1] = bad                                      # the last entry: the strided loop's final round
            norm, coef = run(p, 1.0, None)
            assert (norm == float("inf") and coef == 0.0) if bad == float("inf") else (norm != norm and coef != coef), (n, bad, norm, coef)


POSITIONS = {"first_element": (0, 0), "a_chunk_of_one": (KINDS.index("f32", 5), 4096), "last_of_the_last": (len(KINDS) - 1, 514),
             "unaligned_view": (IDX["view"], 4098), "bf16_gradient": (IDX["g_bf16"], 7), "f16_gradient": (IDX["g_f16"], 7)}


@pytest.mark.parametrize("position", list(POSITIONS))
@pytest.mark.parametrize("route", ["plain", "clipped"])
def test_one_bad_gradient_element_anywhere_skips_the_whole_step(route, position):
    """DeviceGradScaler; plain: k_found_inf raises the flag, clipped: k_grad_sqnorm does.  finite, then +inf, -inf and nan
    each followed by a finite step.  A skipped step leaves every parameter, moment and shadow, `step` and the EMA update
    count as they were and halves the scale; the next finite step is inside the bound again."""
    from src.training.fused_adamw import DeviceGradScaler
    ti, ei = POSITIONS[position]
    assert SHAPES[ti] == (4097,) or position != "a_chunk_of_one"
    a = _params(3)
    # 0.5: the finite steps carry the gradient scales 1 and 0.01 (norms ~ 0.67 and ~ 0.007), so the clip engages on two of them
    oa = _opt(a, max_grad_norm=0.5 if route == "clipped" else None, ema_decay=0.9, ema_tau=3.0)
    oa.ema_prepare()
    amp = oa.device_amp = DeviceGradScaler("cuda", init_scale=4096.0, growth_interval=1000)
    worst, t, clipped = so.Worst(), 0, []
    for s, poison in enumerate([None, float("inf"), None, float("-inf"), None, float("nan"), None]):
        sc = amp.get_scale()
        vals = _stored(so.grad_values(SHAPES, 700 + s, s), sc)
        if poison is not None:
            vals[ti].view(-1)[ei] = poison
        before = _state64(oa, a)
        shadows = [oa.ema_shadow(p).clone() for p in a]
        _give(a, vals)
        oa.step()
        if poison is not None:
            after = _state64(oa, a)
            for i in range(len(a)):
                assert all(torch.equal(x, y) for x, y in zip(after[i], before[i])), (s, "state", i)
                assert torch.equal(oa.ema_shadow(a[i]), shadows[i]), (s, "shadow", i)
            assert amp.last_step_skipped() and amp.get_scale() == 0.5 * sc
        else:
            t += 1
            gs = so.f32(float(oa.last_clip_coef) / sc) if route == "clipped" else 1.0 / sc     # sc: a power of two
            clipped.append(route == "clipped" and float(oa.last_clip_coef) < 1.0)
            _check_step(oa, a, before, vals, gs, so.HYPER, t, (route, position, s), worst)
            assert not amp.last_step_skipped() and amp.get_scale() == sc
            assert any(not torch.equal(oa.ema_shadow(p), e) for p, e in zip(a, shadows))
        assert float(oa.state[a[0]]["step"]) == t == float(oa.ema_updates)
    assert t == 4 and amp.get_scale() == 512.0 and clipped == [route == "clipped", False] * 2
    _report(f"skip {route} {position}", worst)


def test_amp_update_directly_against_torch_on_the_cpu():
    """yolo_amp_update_scale on state = [scale, found_inf, last_found_inf] and the tracker, against torch._amp_update_scale_ on
    CPU tensors for the same sequences (dyadic factors: torch multiplies by the double, the kernel by the fp32 factor)."""
    from src.hipops import lib
    from src.hipops.ops import _p, _stream

    def follow(scale, tracker, founds, growth, backoff, interval):
        state = torch.tensor([scale, 0.0, 0.0], device="cuda")
        trk = torch.tensor([tracker], dtype=torch.int32, device="cuda")
        seen = []
        for f in founds:
            state[1] = float(f)
            lib.call("yolo_amp_update_scale", _p(state), _p(trk), growth, backoff, interval, _stream(state))
            scale, tracker = so.amp_update_ref(scale, tracker, f, growth, backoff, interval)
            s = state.cpu()
            assert (float(s[0]), int(trk)) == (scale, tracker), (founds, f, s, int(trk), scale, tracker)
            assert float(s[1]) == 0.0 and float(s[2]) == float(f)       # found_inf handed on and cleared
            seen.append((scale, tracker))
        return seen

    assert follow(1024.0, 0, [0, 0, 0, 0, 1, 0, 0, 0], 2.0, 0.5, 3) == \
        [(1024.0, 1), (1024.0, 2), (2048.0, 0), (2048.0, 1), (1024.0, 0), (1024.0, 1), (1024.0, 2), (2048.0, 0)]
    assert follow(1536.0, 0, [0, 0, 1, 0], 1.5, 0.25, 1) == [(2304.0, 0), (3456.0, 0), (864.0, 0), (1296.0, 0)]
    assert follow(2.0 ** 127, 0, [0, 0], 2.0, 0.5, 1) == [(2.0 ** 127, 0)] * 2              # growing into inf is refused
    assert follow(2.0 ** 127, 1, [0, 0, 1], 2.0, 0.5, 2) == [(2.0 ** 127, 0), (2.0 ** 127, 1), (2.0 ** 126, 0)]
    state = torch.tensor([1024.0, 1.0, 0.0], device="cuda")
    trk = torch.tensor([2], dtype=torch.int32, device="cuda")
    for growth, backoff, interval in ((0.5, 0.5, 3), (2.0, 0.0, 3), (2.0, 1.5, 3), (2.0, 0.5, 0), (float("nan"), 0.5, 3)):
        assert lib.query("yolo_amp_update_scale", _p(state), _p(trk), growth, backoff, interval, _stream(state)) == YOLO_ERR_ARG
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [1024.0, 1.0, 0.0] and int(trk) == 2
