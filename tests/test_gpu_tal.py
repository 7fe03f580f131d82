"""-m gpu: the kernels of csrc/loss_tal.hip (k_tal_decode, k_tal_topk, k_tal_resolve, k_tal_final) through YoloTALoss's
leaf, held stage by stage to the float64 reference of tests/tal_ref.py and the derived limits of tests/strict_tal.py, from
the buffers the launch itself left in its workspace.

Shapes: the anchors and strides of a 64 x 64 input (A = 84) and of a 96 x 64 input (A = 126, not a multiple of 64; scalar
packets in 16 bit and in fp32), N in {1, 3}, nc in {1, 4, 80}, all three dtypes.  The built target sets (strict_tal.make_case,
every property asserted on the CPU when the case is made): a GT with more than topk candidates on all three levels, GTs with
1, 2 and 3 candidates, a GT that contains no anchor point, two overlapping GTs that contest anchors, two identical rows (the
lower owns everything), an exact metric tie at mirror-image anchors with identical logits; an empty image among full ones, a
batch with no GT at all, StaticTargets with spare rows full of garbage, topk = 13 and topk = 1, grad_scale, the three
non-finite variants of the definition's item 10; one run at the step's own shape; bit-identity of two launches; the same
`out` without the gradient; a captured step replayed on three target sets against the eager step."""
import pytest
import torch

import strict_compare as sc
import strict_tal as st
import tal_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, HF = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]
NANO = dict(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256])


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    yield
    print("\n" + sc.report())


def test_yolo_ta_loss_exists():
    from src.model.losses import YoloTALoss
    assert YoloTALoss(num_classes=4).topk == 10


def launch(case, want_grad=True, grad_scale="case"):
    """-> State: out, dpreds and the workspace buffers on the CPU, as the launch left them"""
    from src.hipops import ops as o
    from src.model.losses import PackedTargets, StaticTargets
    gts = [g.to(DEV) for g in case.gts]
    live = sum(g.shape[0] for g in gts)
    if case.capacity is None:
        pk = PackedTargets(gts, DEV)
    else:
        pk = StaticTargets(case.N, case.capacity, DEV)
        assert case.capacity > live and pk.load(case.gts)
        torch.cuda.synchronize()
        junk = torch.tensor([float("nan"), -1e30, 3e38, float("inf"), 1e9], device=DEV)
        pk.gt[live:] = junk                                       # spare rows: the kernels must never look at them
        pk.gt_img[live:] = 12345
    gs = case.grad_scale if grad_scale == "case" else grad_scale
    gsd = None if gs is None else torch.tensor([gs], dtype=F32, device=DEV)
    hy = case.hyper
    out, dp, ws = o.loss_tal_fwd_bwd(case.preds.to(DEV), case.anchors.to(DEV), case.strides.to(DEV), *pk.as_tuple(), case.nc,
                                     hy["topk"], hy["alpha"], hy["beta"], hy["box"], hy["cls"], hy["dfl"], want_grad, gsd)
    torch.cuda.synchronize()
    views = {k: v.cpu() for k, v in o.loss_tal_workspace_views(ws, case.N, case.A, pk.as_tuple()[3]).items()}
    return st.State.from_views(views, live, out.cpu(), None if dp is None else dp.cpu())


def same_state(a, b):
    return torch.equal(a.out, b.out) and torch.equal(a.pbox, b.pbox) and a.lists == b.lists and torch.equal(a.owner, b.owner) and \
        torch.equal(a.label, b.label) and torch.equal(a.t, b.t) and a.tss == b.tss


def full_check(case):
    s = launch(case)
    st.verify(case, s)
    s2 = launch(case)                                             # two launches: bit-identical
    assert same_state(s, s2) and torch.equal(s.dp.view(torch.uint8), s2.dp.view(torch.uint8))
    s3 = launch(case, want_grad=False)                            # validation: the same scalars without the gradient
    assert s3.dp is None and same_state(s, s3)
    s4 = launch(case, grad_scale=None if case.grad_scale is not None else 1024.0)
    assert torch.equal(s.out, s4.out)                             # the loss value is never scaled
    return s


SHAPES = [(n, w, nc) for w in (64, 96) for n in (1, 3) for nc in (1, 4, 80)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-w{s[1]}-nc{s[2]}")
def test_every_stage_within_its_limit(shape, dtype):
    n, w, nc = shape
    case = st.make_case(n, w, nc, dtype)
    s = full_check(case)
    i, r1, r2 = case.props["twins"]                               # the lower of two identical rows owns everything
    off = sum(g.shape[0] for g in case.gts[:i])
    assert int((s.owner[i] == off + r2).sum()) == 0 and int((s.owner[i] == off + r1).sum()) > 0
    i, r, k1, k2 = case.props["tie"]                              # the exact tie: the lower anchor first
    off = sum(g.shape[0] for g in case.gts[:i])
    lst = s.lists[off + r]
    assert [q[0] for q in lst[:2]] == [k1, k2] and lst[0][1] == lst[1][1]
    i, r = case.props["none"]
    assert s.lists[sum(g.shape[0] for g in case.gts[:i]) + r] == []


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("topk", [13, 1])
def test_other_topk(topk, dtype):
    case = st.make_case(3, 96, 4, dtype, hyper=dict(topk=topk), seed=2)
    s = full_check(case)
    i, r = case.props["many"]
    assert len(s.lists[sum(g.shape[0] for g in case.gts[:i]) + r]) == topk
    if topk == 1:                                                 # the tie decides membership: the lower anchor is the one chosen
        i, r, k1, k2 = case.props["tie"]
        assert [q[0] for q in s.lists[sum(g.shape[0] for g in case.gts[:i]) + r]] == [k1]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("empty", [(1,), (0,), (2,)], ids=lambda e: f"empty{e[0]}")
def test_an_empty_image_among_full_ones(empty, dtype):
    case = st.make_case(3, 64, 4, dtype, empty=empty, seed=3)
    s = full_check(case)
    assert int((s.label[empty[0]] >= 0).sum()) == 0 and not bool(s.dp[empty[0], :64].any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_batch_with_no_gt_at_all(dtype):
    case = st.make_case(3, 96, 4, dtype, empty=(0, 1, 2), seed=4)
    s = full_check(case)
    assert s.tss == 1.0 and float(s.out[1]) == 0.0 == float(s.out[3]) and not bool(s.dp[:, :64].any())
    x = case.preds.double()[:, 64:]
    want = tr.bce(x, torch.zeros_like(x)).sum()                   # only BCE at target 0 remains
    assert abs(float(s.out[2]) - float(want)) <= 1e-5 * float(want) and abs(float(s.out[0]) - 0.5 * float(want)) <= 1e-5 * float(want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_static_targets_with_garbage_in_the_spare_rows(dtype):
    case = st.make_case(3, 64, 4, dtype, seed=5)
    s = launch(case)
    case.capacity = case.gt.shape[0] + 9
    s_static = full_check(case)
    assert same_state(s, s_static) and torch.equal(s.dp.view(torch.uint8), s_static.dp.view(torch.uint8))


@pytest.mark.parametrize("dtype,scale", [(HF, 65536.0), (BF, 1024.0)], ids=["f16-65536", "bf16-1024"])
def test_grad_scale_every_element_at_the_scaled_magnitude(dtype, scale):
    case = st.make_case(3, 96, 4, dtype, grad_scale=scale, seed=6)
    s = full_check(case)
    assert bool(torch.isfinite(s.dp.float()).all())
    if dtype == HF:                                               # values that would be subnormal or zero without the scale
        s1 = launch(case, grad_scale=None)
        assert int(((s1.dp.float().abs() < 6e-5) & (s.dp.float() != 0)).sum()) > 100


def _non_finite_case(dtype, variant):
    case = st.make_case(3, 64, 4, dtype, seed=7)
    asg, _ = st.reference(case)
    p = case.preds.float().clone()
    hit = 1
    rows = [j for j in range(case.gt.shape[0]) if int(case.img[j]) == hit]
    pos = (asg["owner"][hit] >= 0).nonzero().flatten()
    a_pos = int(pos[0])
    a_free = int((asg["owner"][hit] < 0).nonzero()[0])
    where = {}
    if variant == "cls":                                          # NaN / +-inf class logits: at a positive's own label, elsewhere
        lab = int(asg["label"][hit, a_pos])
        p[hit, 64 + lab, a_pos] = float("inf")
        p[hit, 64 + (lab + 1) % case.nc, int(pos[1])] = float("nan")
        p[hit, 64, a_free] = float("-inf")
        j = rows[0]                                               # a NaN at a candidate's logit of the row's label: never chosen
        cand = asg["cand"][j].nonzero().flatten()
        p[hit, 64 + int(case.gt[j, 4]), int(cand[-1])] = float("nan")
        where["nan_candidate"] = (j, int(cand[-1]))
    elif variant == "box_positive":                               # a non-finite box at an anchor the clean reference makes a positive
        p[hit, 3, a_pos] = float("nan")
        p[hit, 40, int(pos[1])] = float("inf")
        where["anchors"] = [a_pos, int(pos[1])]
    else:                                                         # a non-finite box at an anchor nobody owns
        p[hit, 20, a_free] = float("nan")
        where["anchors"] = [a_free]
    bad = st.Case(p, case.anchors.float(), case.strides.float(), case.gts, case.nc, dtype, case.what + " non-finite " + variant)
    return bad, hit, where


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["cls", "box_positive", "box_unowned"])
def test_a_non_finite_input_never_becomes_a_finite_gradient(variant, dtype):
    """Item 10 of the definition.  The NaN pattern of dpreds is exactly the rule's (check_values asserts equality of the two
    patterns before it compares the finite elements, of EVERY image, with the limits); the discrete stages hold with the
    poisoned anchors left out of the candidates; every index stayed in range by construction."""
    case, hit, where = _non_finite_case(dtype, variant)
    s = launch(case)
    st.check_topk(case, s), st.check_owner(case, s), st.check_target(case, s)
    st.check_values(case, s, families=("tal_dense", "tal_box"))
    nan = torch.isnan(s.dp.float())
    others = [i for i in range(case.N) if i != hit]
    assert not bool(nan[others].any()) and bool(torch.isfinite(s.dp.float()[others]).all())
    if variant == "cls":
        assert int(nan.sum()) == 4 and not bool(nan[:, :64].any()) and not bool(torch.isfinite(s.out[0]))
        j, a = where["nan_candidate"]
        assert a not in [q[0] for q in s.lists[j]]
    else:
        for a in where["anchors"]:
            assert bool(nan[hit, :64, a].all()) and int(s.label[hit, a]) == -2 and int(s.owner[hit, a]) == -1
            assert all(a not in [q[0] for q in lst] for j, lst in enumerate(s.lists) if int(case.img[j]) == hit)
        assert int(nan.sum()) == 64 * len(where["anchors"])
    s2 = launch(case)
    assert torch.equal(s.dp.view(torch.uint8), s2.dp.view(torch.uint8))


def test_random_batch_at_the_step_shape():
    """A = 8400 (a 640 x 640 input), N = 2, nc = 80, bf16, random: vector packets, every loop of the scan and of the dense
    pass more than once, more than 64 anchors per lane"""
    case = st.make_case(2, 640, 80, BF, h=640, built=False, fill=12, seed=8)
    assert case.A == 8400
    s = full_check(case)
    assert int((s.label >= 0).sum()) > 100


def test_captured_step_on_new_target_sets_equals_eager_steps():
    """the existing captured-step test (tests/test_gpu_train_loop.py) with YoloTALoss: the smallest preset, 160 x 160 inputs,
    StaticTargets refilled between replays; three replays against a twin stepped eagerly, the same tolerances"""
    from src.model.losses import YoloTALoss
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
    crit = YoloTALoss(num_classes=80)
    oa, ob = HipAdamW(a.parameters(), lr=1e-4, weight_decay=1e-2), HipAdamW(b.parameters(), lr=1e-4, weight_decay=1e-2)
    ra = TrainStepRunner(a, crit, oa, "float32", use_graph=True)
    ra.capture_for_batches(*batches[0], boxes_per_image=8, warmup=1)
    rb = TrainStepRunner(b, crit, ob, "float32", use_graph=False)
    rb._eager_step(batches[0][0], [t.cuda() for t in batches[0][1]])
    losses = []
    for img, gts in batches[1:]:
        la = ra.step_batch(img, gts)
        assert la is not None
        lb, ld = rb._eager_step(img, [t.cuda() for t in gts])
        losses.append((float(la.detach()), float(lb.detach())))
        assert set(ld.keys()) == {"total_loss", "box_loss", "cls_loss", "dfl_loss"}
    torch.cuda.synchronize()
    assert ra.scalars.numel() == 4
    for k, (x, y) in enumerate(losses):
        assert x == x and abs(x) < float("inf") and abs(x - y) <= (1e-4 if k == 0 else 5e-3) * abs(y) + 1e-5, losses
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert bool(torch.isfinite(p).all()) and float((p - q).abs().max()) <= 4e-4, (n, float((p - q).abs().max()))
    moved = max(float((p - q0).abs().max()) for p, q0 in zip(a.parameters(), start))
    assert moved > 2e-4, "the captured steps did not update the weights"


@pytest.mark.parametrize("precision", ["bfloat16", "float16"])
def test_module_forward_backward_and_validation(precision):
    """YoloTALoss as a module: list of tensors in, (loss, dict) out, the gradient reaches preds; under no_grad the same value"""
    from src.model.losses import YoloTALoss
    dtype = BF if precision == "bfloat16" else HF
    case = st.make_case(3, 96, 4, dtype, seed=9)
    crit = YoloTALoss(num_classes=4)
    preds = case.preds.to(DEV).requires_grad_(True)
    loss, ld = crit(preds, [g.to(DEV) for g in case.gts], case.anchors.to(DEV), case.strides.to(DEV))
    loss.backward()
    s = launch(case)
    assert torch.equal(preds.grad.cpu(), s.dp) and float(loss) == float(s.out[0])
    assert [ld[k] for k in ("total_loss", "box_loss", "cls_loss", "dfl_loss")] == s.out.tolist()
    with torch.no_grad():
        loss2, _ = crit(case.preds.to(DEV), [g.to(DEV) for g in case.gts], case.anchors.to(DEV), case.strides.to(DEV))
    assert float(loss2) == float(loss)
