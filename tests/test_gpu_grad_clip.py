"""-m gpu: global-norm gradient clipping inside HipAdamW.step (`max_grad_norm`; csrc/optim.hip k_grad_sqnorm /
k_clip_finalize, the coefficient applied in flight by k_adamw) against torch.nn.utils.clip_grad_norm_ followed by
torch.optim.AdamW: the norm itself, eager steps, two groups, both loss-scaling routes, a captured graph whose threshold
changes between replays, and the captured model step (one graph, and graph C of the staged data-parallel step)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
NANO = dict(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256])

# test_gpu_optim.py's shapes + an unaligned gradient view, a bf16 `lowp_grad` and a parameter without gradient
SHAPES = [(64, 32, 3, 3), (64,), (7,), (128, 64, 1, 1), (1,), (5000,), (4099,), (300,), (33,)]
VIEW, LOWP, NOGRAD = 6, 7, 8
STD = 0.004                    # 36 095 gradient elements: norm ~ 0.76 * scale, so scales 1 / 0.01 pass a threshold of 1, 30 / 5 do not
SCALES = (1.0, 30.0, 0.01, 5.0)          # a constant scale would be invisible to Adam, which is scale-invariant
NORM_RTOL = 2e-6               # <= 32 fp32 roundings of non-negative terms per partial (32 * 2^-24 = 1.9e-6 on the sum of
#                                squares, half of it under the root) + the double finalize and one fp32 store (< 1e-7)
P_TOL, M_TOL, V_TOL = dict(rtol=1e-5, atol=1e-6), dict(rtol=1e-5, atol=1e-7), dict(rtol=1e-5, atol=1e-9)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).cuda().requires_grad_(True) for s in SHAPES]


def _grad_values(seed, scale):
    """The gradient VALUES of one step as the kernel sees them (fp32 on the host; the LOWP one already rounded to bf16)."""
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(*s, generator=g) * (STD * scale) for s in SHAPES]
    vals[LOWP] = vals[LOWP].bfloat16().float()
    vals[NOGRAD] = None
    return vals


def _give(ps, vals, native):
    """native: the layouts HipAdamW must cope with (a view one element into a larger buffer: 4-byte aligned only; a bf16
    lowp_grad of an fp32 parameter); else plain fp32 .grad tensors for the torch twin."""
    for i, (p, v) in enumerate(zip(ps, vals)):
        if v is None:
            p.grad = None
        elif native and i == VIEW:
            buf = torch.zeros(v.numel() + 1, device="cuda")
            buf[1:].copy_(v)
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4
        elif native and i == LOWP:
            p.grad, p.lowp_grad = None, v.bfloat16().cuda()
        else:
            p.grad = v.cuda()


def _norm64(vals):
    return float(torch.sqrt(sum((v.double() ** 2).sum() for v in vals if v is not None)))


def _close(x, y, what, rtol, atol):
    assert torch.allclose(x, y, rtol=rtol, atol=atol), (what, float((x - y).abs().max()))


def _compare(opt_a, a, opt_b, b, tag=""):
    for i, (x, y) in enumerate(zip(a, b)):
        _close(x, y, (tag, "param", i), **P_TOL)
        if i != NOGRAD:
            _close(opt_a.state[x]["exp_avg"], opt_b.state[y]["exp_avg"], (tag, "exp_avg", i), **M_TOL)
            _close(opt_a.state[x]["exp_avg_sq"], opt_b.state[y]["exp_avg_sq"], (tag, "exp_avg_sq", i), **V_TOL)


def test_norm_matches_the_float64_norm_of_the_same_gradients():
    from src.training.fused_adamw import HipAdamW
    a = _params(0)
    oa = HipAdamW(a, lr=1e-3, max_grad_norm=1.0)
    for s, scale in enumerate(SCALES):
        vals = _grad_values(100 + s, scale)
        _give(a, vals, native=True)
        oa.step()
        want, got = _norm64(vals), float(oa.last_grad_norm)
        print(f"\n[grad norm] scale {scale}: device {got:.9g}  float64 {want:.9g}  rel {abs(got - want) / want:.2e}")
        assert abs(got - want) <= NORM_RTOL * want, (scale, got, want)
        coef = float(oa.last_clip_coef)
        assert coef == 1.0 if want < 0.99 else abs(coef - 1.0 / (want + 1e-6)) <= 4e-6 * coef
    assert oa.last_grad_norm.dim() == 0 and oa.last_grad_norm.is_cuda and oa.last_clip_coef.dim() == 0


def test_follows_clip_grad_norm_then_torch_adamw_over_steps_and_an_lr_change():
    from src.training.fused_adamw import HipAdamW
    a, b, c = _params(1), _params(1), _params(1)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    oa, ob, oc = HipAdamW(a, max_grad_norm=1.0, **kw), torch.optim.AdamW(b, **kw), HipAdamW(c, **kw)
    clipped = []
    for s in range(6):
        if s == 3:
            for o in (oa, ob, oc):
                o.param_groups[0]["lr"] = 2.5e-4
        vals = _grad_values(200 + s, SCALES[s % 4])
        _give(a, vals, True), _give(b, vals, False), _give(c, vals, True)
        before = [None if p.grad is None else p.grad.clone() for p in a]
        oa.step(), oc.step()
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ob.step()
        norm, coef = _norm64(vals), float(oa.last_clip_coef)
        assert abs(norm - 1.0) > 0.05                       # no step sits on the threshold
        assert (coef < 1.0) if norm > 1.0 else (coef == 1.0), (s, norm, coef)
        clipped.append(norm > 1.0)
        # the one deviation from clip_grad_norm_: the gradients themselves are left alone
        assert all(x is None or torch.equal(x, p.grad) for x, p in zip(before, a))
    assert clipped == [False, True, False, True, False, True]
    _compare(oa, a, ob, b)
    assert float(oa.state[a[0]]["step"]) == 6
    # the clip engaged: an unclipped run ends elsewhere by more than the tolerances
    assert any(not torch.allclose(x, z, **P_TOL) for x, z in zip(a, c))
    assert any(not torch.allclose(oa.state[x]["exp_avg"], oc.state[z]["exp_avg"], **M_TOL)
               for i, (x, z) in enumerate(zip(a, c)) if i != NOGRAD)


def test_a_threshold_never_reached_is_bit_identical_to_no_clipping():
    from src.training.fused_adamw import HipAdamW
    a, b = _params(2), _params(2)
    oa, ob = HipAdamW(a, lr=1e-3, weight_decay=1e-2, max_grad_norm=1e30), HipAdamW(b, lr=1e-3, weight_decay=1e-2)
    for s in range(4):
        vals = _grad_values(300 + s, SCALES[s])
        _give(a, vals, True), _give(b, vals, True)
        oa.step(), ob.step()
        assert float(oa.last_clip_coef) == 1.0
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
        if i != NOGRAD:
            assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"]), i
            assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"]), i


def test_two_parameter_groups_share_one_global_norm():
    from src.training.fused_adamw import HipAdamW
    a, b = _params(3), _params(3)
    groups = lambda ps: [dict(params=ps[:4], lr=1e-3), dict(params=ps[4:], lr=3e-4, weight_decay=0.0)]
    oa = HipAdamW(groups(a), weight_decay=1e-2, max_grad_norm=1.0)
    ob = torch.optim.AdamW(groups(b), weight_decay=1e-2)
    for s in range(6):
        vals = _grad_values(400 + s, SCALES[s % 4])
        _give(a, vals, True), _give(b, vals, False)
        oa.step()
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ob.step()
        want = _norm64(vals)                                # ONE norm over both groups
        assert abs(float(oa.last_grad_norm) - want) <= NORM_RTOL * want
    _compare(oa, a, ob, b)
    assert all("max_grad_norm" not in g for g in oa.param_groups)


@pytest.mark.parametrize("route", ["device_scaler", "gradscaler_protocol"])
def test_under_loss_scaling_the_norm_is_of_the_unscaled_gradients(route):
    """finite, inf, finite, nan, finite, finite with growth_interval 2 (the sequence of test_gpu_optim.py's scaler test);
    torch side: unscale_, clip_grad_norm_, step, update.  `device_scaler`: DeviceGradScaler, where the norm pass also
    raises found_inf; `gradscaler_protocol`: torch's GradScaler stepping HipAdamW through grad_scale / found_inf."""
    from src.training.fused_adamw import DeviceGradScaler, HipAdamW
    a, b = _params(4), _params(4)
    oa = HipAdamW(a, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    ob = torch.optim.AdamW(b, lr=1e-3, weight_decay=1e-2)
    ref = torch.amp.GradScaler("cuda", init_scale=4096.0, growth_interval=2)
    ref.scale(torch.zeros(1, device="cuda"))
    if route == "device_scaler":
        mine = oa.device_amp = DeviceGradScaler("cuda", init_scale=4096.0, growth_interval=2)
    else:
        mine = torch.amp.GradScaler("cuda", init_scale=4096.0, growth_interval=2)
        mine.scale(torch.zeros(1, device="cuda"))
    poison = {1: float("inf"), 3: float("nan")}
    skipped = []
    for s in range(6):
        sc = ref.get_scale()
        assert mine.get_scale() == sc, (s, mine.get_scale(), sc)
        unscaled = _grad_values(500 + s, SCALES[s % 4])
        vals = [None if v is None else v * sc for v in unscaled]          # gradients of the scaled loss (sc: a power of two)
        vals[LOWP] = vals[LOWP].bfloat16().float()
        if s in poison:
            vals[2][3] = poison[s]
        _give(a, vals, True), _give(b, vals, False)
        before = [p.detach().clone() for p in a]
        if route == "device_scaler":
            oa.step()
        else:
            mine.step(oa)
            mine.update()
        ref.unscale_(ob)
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ref.step(ob)
        ref.update()
        for i, (x, y) in enumerate(zip(a, b)):
            _close(x, y, (s, "param", i), **P_TOL)
        skip = all(torch.equal(x, y) for x, y in zip(a, before))
        if route == "device_scaler":
            assert mine.last_step_skipped() == skip
        skipped.append(skip)
        got = float(oa.last_grad_norm)
        if s in poison:
            assert skip and (got != got or got == float("inf")), (s, got)
        else:
            want = _norm64(vals) / sc
            assert abs(got - want) <= NORM_RTOL * want, (s, got, want)
    assert skipped == [False, True, False, True, False, False]
    assert mine.get_scale() == ref.get_scale() == 2048.0
    assert float(oa.state[a[0]]["step"]) == 4 == float(ob.state[b[0]]["step"])


def test_inside_a_captured_graph_with_a_threshold_change_between_replays():
    """Five replays on regenerated gradients whose norms straddle the threshold, which drops from 1 to 0.25 between
    replays 2 and 3 through sync_hyper() (no recapture).  Parameters against the torch twin and the norm after every
    replay; two identical sequences from the same start are bit-identical (no float atomics anywhere in the pass)."""
    from src.training.fused_adamw import HipAdamW
    stds = [0.004, 0.02, 0.004, 0.002, 0.001]               # norms ~ 0.76, 3.8, 0.76 | 0.38, 0.19 against 1, 1, 1 | 0.25, 0.25
    want_clipped = [False, True, False, True, False]

    def run(check):
        a, b = _params(5), _params(5)
        oa = HipAdamW(a, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
        ob = torch.optim.AdamW(b, lr=1e-3, weight_decay=0.0)
        static = [torch.zeros(*s, device="cuda") for s in SHAPES]

        def produce(ps, native):               # fresh gradient tensors every time (like autograd), values from `static`
            for i, (p, s) in enumerate(zip(ps, static)):
                if i == NOGRAD:
                    p.grad = None
                elif native and i == VIEW:
                    buf = torch.zeros(s.numel() + 1, device="cuda")
                    buf[1:].copy_(s)
                    p.grad = buf[1:]
                elif native and i == LOWP:
                    p.grad, p.lowp_grad = None, s.bfloat16()
                else:
                    p.grad = s.bfloat16().float() if i == LOWP else s * 1.0

        gen = torch.Generator(device="cuda").manual_seed(6)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for s_ in static:
                s_.normal_(generator=gen).mul_(0.004)
            produce(a, True), produce(b, False)
            oa.step()                          # eager warm-up step (allocates tables, state and the clip buffers)
            torch.nn.utils.clip_grad_norm_(b, 1.0)
            ob.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for p in a:
            p.grad = p.lowp_grad = None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            produce(a, True)
            oa.step()
        oa.finish_capture()
        norms, cur = [], 1.0
        for r, std in enumerate(stds):
            if r == 3:
                cur = oa.max_grad_norm = 0.25
                oa.sync_hyper()
            for s_ in static:
                s_.normal_(generator=gen).mul_(std)
            produce(b, False)
            want = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in b if p.grad is not None)))
            g.replay()
            torch.nn.utils.clip_grad_norm_(b, cur)
            ob.step()
            got, coef = float(oa.last_grad_norm), float(oa.last_clip_coef)
            norms.append(oa.last_grad_norm.clone())
            if check:
                assert abs(got - want) <= NORM_RTOL * want, (r, got, want)
                assert ((coef < 1.0) if want_clipped[r] else (coef == 1.0)) and (want > cur) == want_clipped[r], (r, want, coef)
                for i, (x, y) in enumerate(zip(a, b)):
                    _close(x, y, (r, "param", i), **P_TOL)
        torch.cuda.synchronize()
        assert float(oa.state[a[0]]["step"]) == 6
        return [p.detach().clone() for p in a] + norms

    first, second = run(True), run(False)
    assert all(torch.equal(x, y) for x, y in zip(first, second))


# ------------------------------------------------------------------------------------------------ model level
# Relative spread of the UNCLIPPED global gradient norm of the capture batch between two eager runs from identical
# weights (float-atomic BatchNorm statistics; nano, 2x3x160x160, fp32), measured with tools/grad_norm_spread.py on an
# MI355X before these tests first ran: see the docstring of _model_case.  The bound on A's norm against B's is 4x it.
NORM_SPREAD = 4.04e-6
MODEL_NORM_RTOL = 4 * NORM_SPREAD


@pytest.fixture(scope="module")
def pg():
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29561")
    from src.training.distributed_setup import cleanup_distribute_mode, init_distributed_mode
    yield init_distributed_mode("cuda")
    cleanup_distribute_mode()


def _model_case(force_comm):
    """The shape of test_gpu_train_loop.py's test_captured_step_on_new_batches_equals_eager_steps.  Runner A: captured,
    HipAdamW(max_grad_norm=c).  Twin B: eager, clip_grad_norm_(c) on its .grad tensors, then an unclipped HipAdamW.  c is
    half the norm B measures on the capture batch, so the clip is certainly active.

    Norm bound.  Eight eager fwd + bwd of the capture batch from identical weights (the code before clipping existed)
    gave global gradient norms 81.69008596 81.68986704 81.69016555 81.68983535 81.68993097 81.68996728 81.6897119
    81.68980704: the largest difference between two consecutive runs is 4.04e-6 relative (max - min over all eight:
    5.55e-6).  A's device norm must be within 4 x 4.04e-6 = 1.62e-5 of B's float64 norm wherever both see the same batch
    with IDENTICAL weights: the eager warm-up step, and the first captured step, which replays the capture batch after
    B has been given A's weights.  On the later batches the weights have drifted apart by Adam's sign-like update of
    noise-level gradients (that is why the loss is compared at 1e-4 there), so their norms are printed, not bounded."""
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training.fused_adamw import HipAdamW
    from src.training.graph_step import TrainStepRunner
    g = torch.Generator().manual_seed(21)

    def batch(counts):
        img = torch.randn(len(counts), 3, 160, 160, generator=g).cuda()
        gts = [torch.cat([torch.rand(c, 2, generator=g) * 160, torch.rand(c, 2, generator=g) * 60 + 8,
                          torch.randint(0, 80, (c, 1), generator=g).float()], 1) for c in counts]
        return img, gts

    batches = [batch([3, 5]), batch([1, 0]), batch([7, 2]), batch([2, 2])]
    torch.manual_seed(0)
    a = Model(**NANO, num_classes=80).cuda().train()
    b = Model(**NANO, num_classes=80).cuda().train()
    b.load_state_dict(a.state_dict())
    start = [p.detach().clone() for p in a.parameters()]
    crit = YoloDFLQFLoss(num_classes=80)
    ob = HipAdamW(b.parameters(), lr=1e-4, weight_decay=1e-2)
    rb = TrainStepRunner(b, crit, ob, "float32", use_graph=False)

    def eager_b(img, gts, c=None):
        """fwd + bwd, torch's clip on the .grad tensors, unclipped HipAdamW; -> loss, float64 pre-clip norm, threshold"""
        ob.zero_grad(set_to_none=True)
        loss, _ = rb._fwd_bwd(img, [t.cuda() for t in gts])
        norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in b.parameters() if p.grad is not None)))
        c = 0.5 * norm if c is None else c
        torch.nn.utils.clip_grad_norm_(b.parameters(), c)
        ob.step()
        return loss, norm, c

    _, norm0, c = eager_b(*batches[0])                     # the warm-up step on the capture batch sets the threshold:
    oa = HipAdamW(a.parameters(), lr=1e-4, weight_decay=1e-2, max_grad_norm=c)          # half its norm, certainly active
    ra = TrainStepRunner(a, crit, oa, "float32", use_graph=True, force_comm=force_comm)
    ra.capture_for_batches(*batches[0], boxes_per_image=8, warmup=1)
    assert ra.graph is not None and (ra.graph2 is not None) == force_comm and ra.opt_in_graph == (not force_comm)
    got0, coef0 = float(oa.last_grad_norm), float(oa.last_clip_coef)
    print(f"\n[model clip] warm-up: norm A {got0:.8g} B {norm0:.8g} rel {abs(got0 - norm0) / norm0:.2e} coef {coef0:.6f}")
    assert abs(got0 - norm0) <= MODEL_NORM_RTOL * norm0, (got0, norm0)
    assert abs(coef0 - 0.5) < 1e-3
    b.load_state_dict(a.state_dict())                      # identical weights again for the first CAPTURED step
    losses = []
    for k, (img, gts) in enumerate(batches[:1] + batches[1:]):
        la = ra.step_batch(img, gts)
        assert la is not None
        lb, nb, _ = eager_b(img, gts, c)
        na, ca = float(oa.last_grad_norm), float(oa.last_clip_coef)
        losses.append((float(la.detach()), float(lb.detach())))
        print(f"[model clip] replay {k} (batch {k}): norm A {na:.8g} B {nb:.8g} rel {abs(na - nb) / nb:.2e} coef {ca:.6f}")
        if k == 0:
            assert abs(na - nb) <= MODEL_NORM_RTOL * nb, (na, nb)
            assert ca < 0.75                                # c is half the norm of this batch one step earlier
        assert abs(ca - min(1.0, c / (na + 1e-6))) <= 1e-6
    torch.cuda.synchronize()
    # replay 0: identical weights; replay 1 = the first NEW batch, one step after identical weights
    for k in (0, 1):
        assert abs(losses[k][0] - losses[k][1]) <= 1e-4 * abs(losses[k][1]) + 1e-5, losses
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert float((p - q).abs().max()) <= 4e-4, (n, float((p - q).abs().max()))
    moved = max(float((p - q0).abs().max()) for p, q0 in zip(a.parameters(), start))
    assert moved > 2e-4 and all(torch.isfinite(p).all() for p in a.parameters())


def test_captured_model_step_clips_like_clip_grad_norm_on_an_eager_twin():
    _model_case(force_comm=False)


def test_staged_data_parallel_step_clips_inside_graph_c(pg):
    _model_case(force_comm=True)
