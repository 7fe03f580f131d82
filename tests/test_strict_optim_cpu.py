"""No GPU: the proof of tests/strict_optim.py, the comparator of tests/test_gpu_adamw.py.  The unmutated float64 reference IS
torch.optim.AdamW; an fp32 stand-in of the kernel's sequence (last operation fused and unfused) stays inside 1 x the derived
bounds for fp32, bf16 and f16 stores; each of the six mutants leaves 2 x E_p on most of the block meant to show it; and
the finalize / scale-update references are right at their own edges."""
import math

import pytest
import torch
from torch import nn

import strict_optim as so

U = so.U
STEPPED = [i for i, k in enumerate(so.KINDS) if k not in ("nograd", "empty")]


def _stored_grad(i, v):
    """The gradient of tensor i as the kernel reads it (a lowp_grad rounded to its 16-bit type), widened to fp32."""
    return v.to(so.G_DTYPE[so.KINDS[i]]).float() if so.KINDS[i] in so.G_DTYPE else v


def test_the_reference_is_float64_torch_adamw():
    """6 steps from the same state, weight decay 0.1, the lr changed at step 4, zeros among the gradients (the zero run of
    the even steps).  m' is compared at 1e-12 of its mass |b1 m| + |(1-b1) g| (torch forms it as a lerp, m + (1-b1)(g - m):
    where the two terms cancel, the RELATIVE difference of two correct float64 evaluations is not bounded), p' and v' at
    1e-12 relative."""
    lr, b1, b2, eps, wd = so.HYPER
    g0 = torch.Generator().manual_seed(11)
    for i in STEPPED:
        shape = so.SHAPES[i]
        q = nn.Parameter(torch.randn(*shape, generator=g0).double())
        opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
        m = v = torch.zeros(shape, dtype=torch.float64)
        for s in range(6):
            if s == 3:
                lr = opt.param_groups[0]["lr"] = 2.5e-3
            g = so.grad_values([shape], 100 + s, s)[0].double()
            assert s % 2 or shape == (1,) or shape == (3,) or int((g == 0).sum()) >= g.numel() // 8
            p0 = q.detach().clone()
            p1, m1, v1, *_ = so.adamw_ref(p0, g, m, v, 1.0, (lr, b1, b2, eps, wd), s + 1, torch.float32)
            q.grad = g.clone()
            opt.step()
            tm, tv = opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
            assert bool(((q.detach() - p1).abs() <= 1e-12 * p1.abs()).all()), (i, s)
            assert bool(((tm - m1).abs() <= 1e-12 * ((b1 * m).abs() + ((1 - b1) * g).abs())).all()), (i, s)
            assert bool(((tv - v1).abs() <= 1e-12 * v1.abs()).all()), (i, s)
            m, v = tm.clone(), tv.clone()
        lr = so.HYPER[0]


@pytest.fixture(scope="module")
def standin_run():
    """6 steps of the fp32 stand-in over every stepped layout, gs alternating between 1 and fl(fl(1/1536) * fl(0.37)); per
    step and tensor the state before, the gradient as stored, gs, and the fused and unfused results from that state."""
    g0 = torch.Generator().manual_seed(12)
    state = {}
    for i in STEPPED:
        p = torch.randn(*so.SHAPES[i], generator=g0).to(so.P_DTYPE.get(so.KINDS[i], torch.float32))
        state[i] = (p, torch.zeros(so.SHAPES[i]), torch.zeros(so.SHAPES[i]))
    rows = []
    for s in range(6):
        vals = so.grad_values(so.SHAPES, 200 + s, s)
        scale, coef = (None, None) if s % 2 == 0 else (torch.tensor(1536.0), torch.tensor(0.37))
        for i in STEPPED:
            p, m, v = state[i]
            g = _stored_grad(i, vals[i] * (1536.0 if scale is not None else 1.0))
            fused = so.adamw_standin(p, g, m, v, scale, coef, so.HYPER, s + 1, fused=True)
            unfused = so.adamw_standin(p, g, m, v, scale, coef, so.HYPER, s + 1, fused=False)
            rows.append((s, i, (p, m, v), g, fused[3], fused[:3], unfused[:3]))
            state[i] = fused[:3]
    return rows


def _ref(row, mutant=None):
    s, i, (p, m, v), g, gs, _, _ = row
    return so.adamw_ref(p.double(), g.double(), m.double(), v.double(), gs, so.HYPER, s + 1, p.dtype, mutant)


def test_the_fp32_standin_stays_inside_the_bound_fused_and_unfused(standin_run):
    worst = so.Worst()
    gs_seen = set()
    for row in standin_run:
        s, i, _, _, gs, fused, unfused = row
        gs_seen.add(gs)
        p1, m1, v1, e_p, e_m, e_v = _ref(row)
        for tag, (gp, gm, gv) in (("fused", fused), ("unfused", unfused)):
            store = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "f16"}[gp.dtype]
            rp = worst.add(f"E_p[{store},{tag}]", (gp.double() - p1).abs(), e_p)
            rm = worst.add(f"E_m[{tag}]", (gm.double() - m1).abs(), e_m)
            rv = worst.add(f"E_v[{tag}]", (gv.double() - v1).abs(), e_v)
            assert max(rp, rm, rv) <= 1.0, (s, i, tag, rp, rm, rv)
    print(f"\n[strict_optim cpu] worst err / E: {worst}", end="")
    assert len(gs_seen) == 2 and 1.0 in gs_seen
    assert set(k.split("[")[1].split(",")[0] for k in worst.w if k.startswith("E_p")) == {"fp32", "bf16", "f16"}
    # the bound is not slack by orders of magnitude: the fp32 store uses a fair share of it somewhere
    assert worst.w["E_p[fp32,fused]"] > 0.2 and worst.w["E_m[fused]"] > 0.2 and worst.w["E_v[fused]"] > 0.2, worst.w


def test_every_mutant_leaves_twice_the_bound_on_most_of_its_block(standin_run):
    """Against the stand-in's fp32 parameters: the eps mutants on the eps block, the others on all fp32 elements; the best
    step's fraction must exceed one half."""
    fracs = {name: {} for name in so.MUTANTS}
    for row in standin_run:
        s, i, (p, _, _), _, _, fused, _ = row
        if p.dtype != torch.float32 or p.numel() < 8:
            continue
        e_p = _ref(row)[3].flatten()
        got = fused[0].double().flatten()
        for name in so.MUTANTS:
            pm = _ref(row, name)[0].flatten()
            out = (got - pm).abs() > so.HEADROOM * e_p
            blk = so.eps_block(p.numel()) if name in so.EPS_BLOCK_MUTANTS else slice(None)
            k, n = fracs[name].get(s, (0, 0))
            fracs[name][s] = (k + int(out[blk].sum()), n + out[blk].numel())
    for name, per_step in fracs.items():
        best = max(k / n for k, n in per_step.values())
        print(f"\n[strict_optim cpu] mutant {name}: outside 2 E_p on {best:.4f} of its block at its best step", end="")
        assert best > 0.5, (name, per_step)
    assert fracs["step_off"][0][0] == 0             # step 1 has no earlier bias correction: the mutant is the rule there


def test_the_bound_is_finite_and_zero_free_where_the_second_moment_is_zero():
    p = torch.tensor([0.5, -2.0, 0.0], dtype=torch.float64)
    z = torch.zeros(3, dtype=torch.float64)
    p1, m1, v1, e_p, e_m, e_v = so.adamw_ref(p, z, z, z, 1.0, so.HYPER, 1, torch.float32)
    assert torch.equal(m1, z) and torch.equal(v1, z) and torch.equal(p1, p * (1.0 - 1e-2 * 0.1))
    assert bool(torch.isfinite(e_p).all()) and bool((e_p > 0).all()) and bool((e_p[:2] < 8 * U * p.abs()[:2]).all())
    # the store's half ulp at p' = 0.4995 (the binade of 0.25): bf16 2^-10, f16 2^-13, plus the fp32 terms (< 1e-6 of it)
    for dtype, half in ((torch.bfloat16, 2.0 ** -10), (torch.float16, 2.0 ** -13)):
        e = float(so.adamw_ref(p, z, z, z, 1.0, so.HYPER, 1, dtype)[3][0])
        assert half < e < half + 8 * U
    # an f16 parameter at zero is held to half the subnormal spacing 2^-24, not to a relative figure of nothing
    e = float(so.adamw_ref(p, z, z, z, 1.0, so.HYPER, 1, torch.float16)[3][2])
    assert 2.0 ** -25 <= e < 2.0 ** -25 * (1 + 1e-6)


def test_clip_finalize_reference_at_its_edges():
    f = so.clip_finalize_ref
    assert f(torch.zeros(0), 1.0) == (0.0, 1.0)                                  # no partials: norm 0, nothing clipped
    norm, coef = f(torch.tensor([9.0, 16.0]), 10.0)
    assert norm == 5.0 and coef == 1.0
    norm, coef = f(torch.tensor([9.0, 16.0]), 2.5)
    assert norm == 5.0 and coef == 2.5 / (5.0 + 1e-6)
    norm, coef = f(torch.tensor([9.0, 16.0]), 2.5, scale=4.0)                    # the norm of the unscaled gradients
    assert norm == 1.25 and coef == 1.0
    # just under and just over the threshold: norm + 1e-6 against max_norm decides
    assert f(torch.tensor([1.0], dtype=torch.float64), 1.0 + 2e-6)[1] == 1.0
    assert f(torch.tensor([1.0], dtype=torch.float64), 1.0 + 0.5e-6)[1] < 1.0
    assert f(torch.tensor([1.0], dtype=torch.float64), 1.0)[1] == 1.0 / (1.0 + 1e-6)
    norm, coef = f(torch.tensor([1.0, float("inf")]), 1.0)
    assert norm == float("inf") and coef == 0.0
    norm, coef = f(torch.tensor([1.0, float("nan")]), 1.0)
    assert norm != norm and coef != coef
    # and it is clip_grad_norm_'s coefficient
    g = torch.Generator().manual_seed(3)
    ps = [nn.Parameter(torch.zeros(n, dtype=torch.float64)) for n in (5, 4097)]
    for q in ps:
        q.grad = torch.randn(q.shape, generator=g, dtype=torch.float64)
    before = [q.grad.clone() for q in ps]
    total = float(torch.nn.utils.clip_grad_norm_(ps, 3.0))
    norm, coef = f(torch.stack([(b ** 2).sum() for b in before]), 3.0)
    assert abs(norm - total) <= 1e-14 * total and coef < 1.0
    assert all(bool(((q.grad - b * coef).abs() <= 1e-14 * b.abs()).all()) for q, b in zip(ps, before))


def test_sqnorm_reference_and_its_bound():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4096, generator=g) * 0.004
    s, e = so.sqnorm_ref(x)
    assert s == float((x.double() ** 2).sum()) and e == 14 * U * s
    # the accumulation order of k_grad_sqnorm's comment in CPU fp32 (4 accumulators of 4 per lane, then pairwise trees) fits
    lanes = x.view(4, 4, 256)                                       # [it // 4 ... ] any fixed split into 16 per lane will do
    acc = torch.zeros(4, 256)
    for a in range(4):
        for b in range(4):
            acc[b] = so._fma(lanes[a, b], lanes[a, b], acc[b])
    lane = (acc[0] + acc[1]) + (acc[2] + acc[3])
    while lane.numel() > 1:
        lane = lane[0::2] + lane[1::2]
    assert abs(float(lane) - s) <= e
    with pytest.raises(AssertionError):
        so.sqnorm_ref(torch.zeros(4097))


def test_scale_update_reference_at_its_edges():
    f = so.amp_update_ref
    assert f(1024.0, 0, 0, 2.0, 0.5, 1) == (2048.0, 0)                           # interval 1: every clean step grows
    assert f(1024.0, 0, 0, 2.0, 0.5, 3) == (1024.0, 1)
    assert f(1024.0, 1, 0, 2.0, 0.5, 3) == (1024.0, 2)
    assert f(1024.0, 2, 0, 2.0, 0.5, 3) == (2048.0, 0)                           # growth at the interval
    assert f(1024.0, 2, 1, 2.0, 0.5, 3) == (512.0, 0)                            # a backoff resets the tracker
    assert f(2.0 ** 127, 0, 0, 2.0, 0.5, 1) == (2.0 ** 127, 0)                   # growth into inf refused, tracker reset
    assert f(2.0 ** 127, 0, 1, 2.0, 0.5, 1) == (2.0 ** 126, 0)
    assert f(1536.0, 0, 1, 2.0, 0.25, 5) == (384.0, 0)


def test_grad_values_has_the_blocks_the_bounds_need():
    vals = [so.grad_values(so.SHAPES, 5, s) for s in range(4)]
    for s, step_vals in enumerate(vals):
        for shape, v in zip(so.SHAPES, step_vals):
            n = math.prod(shape)
            assert tuple(v.shape) == shape and v.dtype == torch.float32
            if n < 8:
                continue
            f = v.flatten()
            blk = f[so.eps_block(n)].abs()
            assert float(blk.min()) >= 0.99e-10 and float(blk.max()) <= 1.01e-6
            assert bool((f[so.zero_run(n)] == 0).all()) == (s % 2 == 0)
            rest = f[n // 4:].abs()
            assert 0.5 < float(rest.mean()) / (so.STD * so.SCALES[s] * math.sqrt(2 / math.pi)) < 2.0
    assert not torch.equal(vals[0][0], vals[2][0])
