"""-m gpu: the exponential moving average of the weights kept inside HipAdamW.step (`ema_decay` / `ema_tau`;
csrc/optim.hip k_adamw, k_adamw_tick, k_ema_lerp) and `ModelEMA` on top of it: eager steps, that the average does not
change the update, a constant decay and a decay schedule, skipped fp16 steps on both scaling routes, clipping, the buffer
launch, a captured graph whose decay changes between replays, the captured model step (one graph, and graph C of the
staged data-parallel step), the swap for validation and the checkpoint round trip.

The bound.  With x = fl(omd*w) and e' = fl(df*e + x) one step errs by at most 2^-24 (|omd*w| + |e'|), and
earlier error is multiplied by df < 1.  Against the float64 recurrence on the SAME inputs -- the weights read back after
every step, df and omd rounded to fp32 from a float64 d_t -- every element satisfies after T updates
    |e_dev - e_64| <= T * 2^-23 * max(|e_0|, max_t |w_t|).
decay 0.9, tau 3: the average lags the weights by about 1e-3, hundreds of times the bound, and a recurrence whose ramp
index is off by one leaves the bound on nearly every element -- the power check of the first test."""
import math
import os

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
NANO = dict(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256])

# test_gpu_grad_clip.py's set (an unaligned gradient view, a bf16 `lowp_grad`, a parameter without gradient; 4099 and 5000
# cross a chunk boundary with a tail that is no multiple of 4, (1,) and (7,) are degenerate chunks) + a parameter STORED in bf16
SHAPES = [(64, 32, 3, 3), (64,), (7,), (128, 64, 1, 1), (1,), (5000,), (4099,), (300,), (33,), (515,)]
VIEW, LOWP, NOGRAD, BF16P = 6, 7, 8, 9
STD = 0.004
SCALES = (1.0, 30.0, 0.01, 5.0)          # norm ~ 0.76 * scale: 1 / 0.01 pass a clipping threshold of 1, 30 / 5 do not
DECAY, TAU = 0.9, 3.0
EPS = 2.0 ** -23


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(*s, generator=g) for s in SHAPES]
    ps[BF16P] = ps[BF16P].bfloat16()
    return [nn.Parameter(p.cuda()) for p in ps]


def _grad_values(seed, scale):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(*s, generator=g) * (STD * scale) for s in SHAPES]
    vals[LOWP] = vals[LOWP].bfloat16().float()
    vals[BF16P] = vals[BF16P].bfloat16().float()
    vals[NOGRAD] = None
    return vals


def _give(ps, vals):
    for i, (p, v) in enumerate(zip(ps, vals)):
        if v is None:
            p.grad = None
        elif i == VIEW:                     # a view one element into a larger buffer: 4-byte aligned only
            buf = torch.zeros(v.numel() + 1, device="cuda")
            buf[1:].copy_(v)
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4
        elif i == LOWP:                     # a bf16 gradient of an fp32 parameter
            p.grad, p.lowp_grad = None, v.bfloat16().cuda()
        elif i == BF16P:
            p.grad = v.bfloat16().cuda()
        else:
            p.grad = v.cuda()


def _coef(t, decay, tau):
    """(df, omd) as the kernel forms them: fp32 roundings of the float64 d_t and 1 - d_t."""
    d = decay * (1.0 - math.exp(-t / tau)) if tau > 0 else decay
    return float(torch.tensor(d, dtype=torch.float64).float()), float(torch.tensor(1.0 - d, dtype=torch.float64).float())


class Recurrence:
    """The float64 recurrence over a list of tensors, fed the values read back from the device after every update, and
    the same recurrence with the ramp index shifted by one."""

    def __init__(self, start):
        self.e = [t.detach().double().clone() for t in start]
        self.off = [t.detach().double().clone() for t in start]
        self.mx = [t.detach().double().abs() for t in start]
        self.T = 0

    def update(self, live, t, decay, tau, moved=None):
        self.T += 1
        (df, omd), (df1, omd1) = _coef(t, decay, tau), _coef(t + 1, decay, tau)
        for i, w in enumerate(live):
            if moved is not None and not moved[i]:
                continue
            w = w.detach().double()
            self.e[i] = df * self.e[i] + omd * w
            self.off[i] = df1 * self.off[i] + omd1 * w
            self.mx[i] = torch.maximum(self.mx[i], w.abs())

    def check(self, shadows, tag=""):
        """every element inside the bound; -> (largest error / bound, fraction of elements where the shifted recurrence
        leaves the bound)"""
        worst, out, n = 0.0, 0, 0
        for i, s in enumerate(shadows):
            bound = self.T * EPS * self.mx[i]
            err = (s.double() - self.e[i]).abs()
            bad = err > bound
            assert not bool(bad.any()), (tag, i, float(err.max()), float(bound[bad].min()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            out += int(((s.double() - self.off[i]).abs() > bound).sum())
            n += s.numel()
        return worst, out / n


def _shadows(opt, ps):
    return [opt.ema_shadow(p) for p in ps]


MOVED = [i != NOGRAD for i in range(len(SHAPES))]


# ------------------------------------------------------------------------------------------------ optimizer level
def test_eager_steps_follow_the_float64_recurrence_and_an_index_off_by_one_does_not():
    from src.training.fused_adamw import HipAdamW
    a = _params(0)
    oa = HipAdamW(a, lr=1e-3, ema_decay=DECAY, ema_tau=TAU)
    oa.ema_prepare()                        # the shadow of the parameter without gradient exists too
    start = [p.detach().clone() for p in a]
    assert all(torch.equal(e, s.float()) and e.dtype == torch.float32 for e, s in zip(_shadows(oa, a), start))
    rec = Recurrence([s.float() for s in start])
    for s in range(6):
        _give(a, _grad_values(100 + s, SCALES[s % 4]))
        oa.step()
        assert float(oa.ema_updates) == s + 1
        rec.update([p.float() for p in a], s + 1, DECAY, TAU, MOVED)
        worst, off = rec.check(_shadows(oa, a), s)
        print(f"\n[ema eager] step {s + 1}: error / bound {worst:.3f}; off-by-one outside the bound on {off:.4f} of the elements")
    # the power check.  Of the 36 610 elements, 33 have no gradient and 515 are stored in bf16, where a move of 1e-3 is
    # below half an ulp for |w| > 0.5: such an element stands still, its average equals it, and no index can show.
    # Every other element lags its weight by ~1e-3, and the shifted ramp moves it by a tenth of that.
    tell = sum(p.numel() for i, p in enumerate(a) if i not in (NOGRAD, BF16P)) / sum(p.numel() for p in a)
    assert off > 0.99 * tell, off
    lag = max(float((e - p.detach().float()).abs().max()) for i, (e, p) in enumerate(zip(_shadows(oa, a), a)) if i != NOGRAD)
    assert lag > 100 * 6 * EPS * 4, lag
    assert torch.equal(oa.ema_shadow(a[NOGRAD]), start[NOGRAD])
    assert oa.ema_updates.dim() == 0 and oa.ema_updates.is_cuda


def test_the_average_does_not_change_the_update():
    from src.training.fused_adamw import HipAdamW
    a, b = _params(1), _params(1)
    groups = lambda ps: [dict(params=ps[:4], lr=1e-3), dict(params=ps[4:], lr=3e-4, weight_decay=0.0)]
    oa = HipAdamW(groups(a), weight_decay=1e-2, ema_decay=DECAY, ema_tau=TAU)
    ob = HipAdamW(groups(b), weight_decay=1e-2)
    for s in range(4):
        vals = _grad_values(200 + s, SCALES[s])
        _give(a, vals), _give(b, vals)
        oa.step(), ob.step()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
        if i != NOGRAD:
            assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"]), i
            assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"]), i
            assert not torch.equal(oa.ema_shadow(x), x.float()), i      # and the average is not the weights themselves
    assert ob.ema_shadow(b[0]) is None
    assert all("ema" not in k for g in oa.param_groups for k in g) and set(oa.state_dict()) == {"state", "param_groups"}


def test_constant_decay_follows_an_lr_change_and_a_decay_change():
    from src.training.fused_adamw import HipAdamW
    a = _params(2)
    oa = HipAdamW(a, lr=1e-3, ema_decay=0.9, ema_tau=0)
    start = [p.detach().float().clone() for p in a]
    rec, decay = None, 0.9
    for s in range(6):
        if s == 2:
            oa.param_groups[0]["lr"] = 2.5e-4
        if s == 4:
            decay = oa.ema_decay = 0.5
            oa.sync_hyper()
        _give(a, _grad_values(300 + s, SCALES[s % 4]))
        oa.step()
        if rec is None:                     # shadows are created by the first step, as copies of the weights before it
            rec = Recurrence([t for i, t in enumerate(start) if i != NOGRAD])
        rec.update([p.float() for i, p in enumerate(a) if i != NOGRAD], s + 1, decay, 0.0)
        worst, _ = rec.check([oa.ema_shadow(p) for i, p in enumerate(a) if i != NOGRAD], s)
        print(f"\n[ema const] step {s + 1} decay {decay}: error / bound {worst:.3f}")
    assert oa.ema_shadow(a[NOGRAD]) is None and float(oa.ema_updates) == 6


class _Net(nn.Module):
    """The tensor set as a module, with float buffers (16, 1, 4099 elements) and an integer one for ModelEMA."""

    def __init__(self, ps):
        super().__init__()
        self.ps = nn.ParameterList(ps)
        g = torch.Generator().manual_seed(77)
        self.register_buffer("mean", torch.randn(16, generator=g))
        self.register_buffer("one", torch.randn(1, generator=g))
        self.register_buffer("var", torch.rand(4099, generator=g) + 0.5)
        self.register_buffer("count", torch.tensor(3, dtype=torch.int64))

    def float_buffers(self):
        return [self.mean, self.one, self.var]

    def jitter(self, seed):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for b in self.float_buffers():
                b.add_((torch.randn(b.shape, generator=g) * 1e-2).cuda())
            self.count.add_(1)


@pytest.mark.parametrize("route", ["device_scaler", "gradscaler_protocol"])
def test_a_skipped_step_moves_neither_shadows_nor_the_update_count(route):
    """finite, inf, finite, nan, finite, finite (the sequence of the scaler tests), parameters AND buffer shadows.
    torch's GradScaler cannot check a bf16 `.grad` for inf (no such kernel), so on its route the parameter stored in
    bf16 gets no gradient; DeviceGradScaler steps it with the others."""
    from src.training.ema import ModelEMA
    from src.training.fused_adamw import DeviceGradScaler, HipAdamW
    a = _params(4)
    net = _Net(a).cuda()
    oa = HipAdamW(a, lr=1e-3, weight_decay=1e-2)
    ema = ModelEMA(net, oa, decay=DECAY, tau=TAU)
    if route == "device_scaler":
        mine = oa.device_amp = DeviceGradScaler("cuda", init_scale=4096.0, growth_interval=2)
    else:
        mine = torch.amp.GradScaler("cuda", init_scale=4096.0, growth_interval=2)
        mine.scale(torch.zeros(1, device="cuda"))
    live = lambda: [p.float() for p in a] + [b.clone() for b in net.float_buffers()]
    shadows = lambda: _shadows(oa, a) + list(ema._buf_shadows)
    rec = Recurrence(live())
    moved = MOVED + [True] * 3
    moved[BF16P] = route == "device_scaler"
    poison = {1: float("inf"), 3: float("nan")}
    t = 0
    for s in range(6):
        sc = mine.get_scale()
        vals = [None if v is None else v * sc for v in _grad_values(500 + s, SCALES[s % 4])]
        vals[LOWP] = vals[LOWP].bfloat16().float()
        if s in poison:
            vals[2][3] = poison[s]
        if not moved[BF16P]:
            vals[BF16P] = None
        _give(a, vals)
        net.jitter(600 + s)                 # new running statistics: an average that moved would show
        before = [e.clone() for e in shadows()]
        before_w = [p.detach().clone() for p in a]
        if route == "device_scaler":
            oa.step()
        else:
            mine.step(oa)
            mine.update()
        if s in poison:
            assert all(torch.equal(x, y) for x, y in zip(before, shadows())), s
            assert all(torch.equal(x, y) for x, y in zip(before_w, a)), s
        else:
            t += 1
            rec.update(live(), t, DECAY, TAU, moved)
            rec.check(shadows(), s)
            assert not torch.equal(before[-1], shadows()[-1])
        assert float(oa.ema_updates) == t, (s, float(oa.ema_updates))
    assert ema.updates == 4 and mine.get_scale() == 2048.0


def test_with_clipping_the_average_follows_the_clipped_weights():
    from src.training.fused_adamw import HipAdamW
    a, b = _params(5), _params(5)
    oa = HipAdamW(a, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, ema_decay=DECAY, ema_tau=TAU)
    ob = HipAdamW(b, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    oa.ema_prepare()
    rec = Recurrence([p.float() for p in a])
    clipped = []
    for s in range(4):
        vals = _grad_values(700 + s, SCALES[s])
        _give(a, vals), _give(b, vals)
        oa.step(), ob.step()
        clipped.append(float(oa.last_clip_coef) < 1.0)
        rec.update([p.float() for p in a], s + 1, DECAY, TAU, MOVED)
        rec.check(_shadows(oa, a), s)
    assert clipped == [False, True, False, True]
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_buffer_launch_averages_float_buffers_and_leaves_integer_ones_to_the_live_model():
    from src.training.ema import ModelEMA
    from src.training.fused_adamw import HipAdamW
    w = nn.Parameter(torch.randn(7, generator=torch.Generator().manual_seed(8)).cuda())
    net = _Net([w]).cuda()
    opt = HipAdamW([w], lr=1e-3)
    ema = ModelEMA(net, opt, decay=DECAY, tau=TAU)
    assert ema._table["njobs"] == 3 and ema._buf_names == ["mean", "one", "var"]        # the int64 buffer is not in the table
    assert ema._table["nchunks"] == 1 + 1 + 2
    rec = Recurrence([b.clone() for b in net.float_buffers()])
    for s in range(6):
        net.jitter(800 + s)
        w.grad = torch.full((7,), 0.01 * (s + 1), device="cuda")
        opt.step()
        rec.update([b.clone() for b in net.float_buffers()], s + 1, DECAY, TAU)
        worst, off = rec.check(ema._buf_shadows, s)
    print(f"\n[ema buffers] error / bound {worst:.3f}; off-by-one outside the bound on {off:.4f} of the elements")
    assert off > 0.9
    sd = ema.state_dict()
    assert set(sd) == {"ema_state", "updates", "decay", "tau"} and sd["updates"] == 6 and sd["decay"] == DECAY and sd["tau"] == TAU
    assert sd["ema_state"]["count"].dtype == torch.int64 and int(sd["ema_state"]["count"]) == 3 + 6
    assert torch.equal(sd["ema_state"]["var"], ema._buf_shadows[2]) and torch.equal(sd["ema_state"]["ps.0"], opt.ema_shadow(w))
    assert set(sd["ema_state"]) == set(net.state_dict())


def test_inside_a_captured_graph_with_a_decay_change_between_replays():
    """The optimizer step alone is captured; five replays on regenerated gradients; the decay drops from 0.9 to 0.5 between
    replays 2 and 3 through sync_hyper() (no recapture).  The bound after every replay; two identical runs are bit-identical."""
    from src.training.fused_adamw import HipAdamW

    def run(check):
        a = _params(9)
        oa = HipAdamW(a, lr=1e-3, weight_decay=0.0, ema_decay=DECAY, ema_tau=TAU)
        oa.ema_prepare()
        rec = Recurrence([p.float() for p in a])
        static = [torch.zeros(*s, device="cuda") for s in SHAPES]

        def produce():                         # fresh gradient tensors every time (like autograd), values from `static`
            for i, (p, s) in enumerate(zip(a, static)):
                if i == NOGRAD:
                    p.grad = None
                elif i == VIEW:
                    buf = torch.zeros(s.numel() + 1, device="cuda")
                    buf[1:].copy_(s)
                    p.grad = buf[1:]
                elif i == LOWP:
                    p.grad, p.lowp_grad = None, s.bfloat16()
                elif i == BF16P:
                    p.grad = s.bfloat16()
                else:
                    p.grad = s * 1.0

        gen = torch.Generator(device="cuda").manual_seed(10)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for s_ in static:
                s_.normal_(generator=gen).mul_(STD)
            produce()
            oa.step()                          # eager warm-up step: tables, state, shadows, control block
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        rec.update([p.float() for p in a], 1, DECAY, TAU, MOVED)
        if check:
            rec.check(_shadows(oa, a), "warm-up")
        for p in a:
            p.grad = p.lowp_grad = None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            produce()
            oa.step()
        oa.finish_capture()
        decay = DECAY
        for r in range(5):
            if r == 3:
                decay = oa.ema_decay = 0.5
                oa.sync_hyper()
            for s_ in static:
                s_.normal_(generator=gen).mul_(STD * SCALES[r % 4])
            g.replay()
            rec.update([p.float() for p in a], r + 2, decay, TAU, MOVED)
            if check:
                worst, _ = rec.check(_shadows(oa, a), r)
                print(f"\n[ema graph] replay {r} decay {decay}: error / bound {worst:.3f}")
                assert float(oa.ema_updates) == r + 2
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="after a graph capture"):
            oa.ema_decay = None
        return [e.clone() for e in _shadows(oa, a)] + [p.detach().clone() for p in a]

    first, second = run(True), run(False)
    assert all(torch.equal(x, y) for x, y in zip(first, second))


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def pg():
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29563")
    from src.training.distributed_setup import cleanup_distribute_mode, init_distributed_mode
    yield init_distributed_mode("cuda")
    cleanup_distribute_mode()


def _batches():
    """the batches of test_gpu_grad_clip.py's _model_case"""
    g = torch.Generator().manual_seed(21)

    def batch(counts):
        img = torch.randn(len(counts), 3, 160, 160, generator=g).cuda()
        gts = [torch.cat([torch.rand(c, 2, generator=g) * 160, torch.rand(c, 2, generator=g) * 60 + 8,
                          torch.randint(0, 80, (c, 1), generator=g).float()], 1) for c in counts]
        return img, gts
    return [batch([3, 5]), batch([1, 0]), batch([7, 2]), batch([2, 2])]


_CASES = {}


def _model_case(force_comm):
    """Captured TrainStepRunner + ModelEMA on the nano preset, 2x3x160x160, fp32.  After the warm-up step and each of four
    replays every parameter AND every BatchNorm running statistic is read back and every shadow is held to the bound:
    the captured step updates both on every replay, with the right ramp index."""
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training.ema import ModelEMA
    from src.training.fused_adamw import HipAdamW
    from src.training.graph_step import TrainStepRunner
    batches = _batches()
    torch.manual_seed(0)
    model = Model(**NANO, num_classes=80).cuda().train()
    opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    ema = ModelEMA(model, opt, decay=DECAY, tau=TAU)
    stepped = [p for p in model.parameters() if p.requires_grad]
    assert len(stepped) == len(list(model.parameters())) - 1 and opt.ema_shadow(model.head.dfl.conv.weight) is None
    assert len(ema._bufs) > 20 and all(b.dtype == torch.float32 for b in ema._bufs)
    live = lambda: [p.detach().clone() for p in stepped] + [b.clone() for b in ema._bufs]
    shadows = lambda: [opt.ema_shadow(p) for p in stepped] + list(ema._buf_shadows)
    rec = Recurrence(live())
    runner = TrainStepRunner(model, YoloDFLQFLoss(num_classes=80), opt, "float32", use_graph=True, force_comm=force_comm)
    runner.capture_for_batches(*batches[0], boxes_per_image=8, warmup=1)
    assert runner.graph is not None and (runner.graph2 is not None) == force_comm and runner.opt_in_graph == (not force_comm)
    rec.update(live(), 1, DECAY, TAU)
    worst, off = rec.check(shadows(), "warm-up")
    for k, (img, gts) in enumerate(batches):
        assert runner.step_batch(img, gts) is not None
        rec.update(live(), k + 2, DECAY, TAU)
        worst, off = rec.check(shadows(), k)
        print(f"\n[ema model] replay {k}: error / bound {worst:.3f}; off-by-one outside the bound on {off:.4f} of the elements")
        assert ema.updates == k + 2
    assert off > 0.99                       # every trainable parameter and every running statistic moves on every step
    return model, opt, ema, runner, batches


def test_captured_model_step_averages_parameters_and_running_statistics():
    _CASES[False] = _model_case(force_comm=False)


def test_staged_data_parallel_step_averages_inside_graph_c(pg):
    _model_case(force_comm=True)


def test_swap_for_validation_and_back():
    from src.model.model_builder import Model
    model, opt, ema, runner, batches = _CASES.get(False) or _model_case(force_comm=False)
    x = batches[2][0]
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with ema.applied(model):
        with torch.no_grad():
            preds = model.eval()(x)[0].clone()
        inside = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    fresh = Model(**NANO, num_classes=80).cuda()
    fresh.load_state_dict(ema.state_dict()["ema_state"])
    with torch.no_grad():
        want = fresh.eval()(x)[0]
    assert torch.equal(preds, want)
    assert all(torch.equal(inside[k], v) for k, v in fresh.state_dict().items())
    assert any(not torch.equal(inside[k], before[k]) for k in before)
    after = model.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in before)        # bit for bit, parameters and buffers
    # the captured step still replays, on the raw weights, and moves weights and shadows
    w, e = model.net.p2[1].conv2.conv.weight, None
    e = opt.ema_shadow(w)
    w0, e0, bs0, n0 = w.detach().clone(), e.clone(), ema._buf_shadows[0].clone(), ema.updates
    assert runner.step_batch(*batches[1]) is not None
    assert not torch.equal(w, w0) and not torch.equal(e, e0) and not torch.equal(ema._buf_shadows[0], bs0)
    assert ema.updates == n0 + 1


def _synthetic_step(model, opt, seed):
    """the same gradients on both sides (a real backward's float-atomic BatchNorm statistics differ from run to run)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.requires_grad:
                p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3
        for b in model.buffers():
            if b.is_floating_point():
                b.add_(torch.randn(b.shape, generator=g, device="cuda") * 1e-3)
    opt.step()


def test_checkpoint_round_trip(tmp_path, capsys):
    from src.model.model_builder import Model
    from src.training.ema import ModelEMA
    from src.training.fused_adamw import HipAdamW
    from src.training.utils_train import load_checkpoint, save_checkpoint

    def make():
        model = Model(**NANO, num_classes=80).cuda().train()
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
        return model, opt, ModelEMA(model, opt, decay=DECAY, tau=TAU)

    def shadows(model, opt, ema):
        return [opt.ema_shadow(p) for p in model.parameters() if p.requires_grad] + list(ema._buf_shadows)

    torch.manual_seed(1)
    a = make()
    for s in range(3):
        _synthetic_step(a[0], a[1], 900 + s)
    save_checkpoint(a[0], a[1], 1, 0.0, checkpoint_dir=str(tmp_path), ema=a[2])
    ck = torch.load(tmp_path / "model_epoch_1.pth", weights_only=False)
    assert {"ema_state", "ema_updates", "ema_decay", "ema_tau"} <= set(ck) and ck["ema_updates"] == 3
    assert all(torch.equal(ck["model_state"][k].cuda(), v) for k, v in a[0].state_dict().items())     # the raw weights
    torch.manual_seed(2)
    b = make()
    b[2].optimizer.ema_decay = 0.7          # whatever the fresh objects were built with, the checkpoint's values hold
    assert load_checkpoint(b[0], b[1], str(tmp_path / "model_epoch_1.pth"), map_location="cuda", ema=b[2]) == 1
    assert b[2].updates == a[2].updates == 3 and b[2].decay == DECAY and b[2].tau == TAU
    assert all(torch.equal(x, y) for x, y in zip(shadows(*a), shadows(*b)))
    _synthetic_step(a[0], a[1], 950), _synthetic_step(b[0], b[1], 950)
    assert all(torch.equal(x, y) for x, y in zip(shadows(*a), shadows(*b)))
    assert all(torch.equal(x, y) for x, y in zip(a[0].parameters(), b[0].parameters()))
    assert b[2].updates == 4
    # a checkpoint without the keys (an older one, the reference's): the average restarts at the loaded weights
    save_checkpoint(a[0], a[1], 2, 0.0, checkpoint_dir=str(tmp_path))
    assert "ema_state" not in torch.load(tmp_path / "model_epoch_2.pth", weights_only=False)
    c = make()
    _synthetic_step(c[0], c[1], 960)
    capsys.readouterr()
    load_checkpoint(c[0], c[1], str(tmp_path / "model_epoch_2.pth"), map_location="cuda", ema=c[2])
    assert "[INFO]" in capsys.readouterr().out
    assert c[2].updates == 0
    live = [p.detach() for p in c[0].parameters() if p.requires_grad] + list(c[2]._bufs)
    assert all(torch.equal(e, w) for e, w in zip(shadows(*c), live))
    assert all(torch.equal(x, y) for x, y in zip(a[0].parameters(), c[0].parameters()))
