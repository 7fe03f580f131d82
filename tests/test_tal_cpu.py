"""No-GPU checks of the task-aligned loss: a hand-worked case that the float64 reference (tests/tal_ref.py) reproduces, the
reference's invariants on random cases, the proof of the comparator (tests/strict_tal.py: the fp32 CPU stand-in passes, an
output just beyond a family's limit fails and one just inside passes, a chosen set with one wrong member fails), and the
script's reading of `training.loss`.  The kernels are covered by tests/test_gpu_tal.py."""
import copy
import importlib.util
import math
import os

import pytest
import torch

import strict_compare as sc
import strict_tal as st
import tal_ref as tr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F32, F64, BF, HF = torch.float32, torch.float64, torch.bfloat16, torch.float16
STAND_IN_MAXIMA = """the fp32 stand-in, the six cases of test_stand_in_has_nothing_outside, 2026-10-19: loss_decode 0.126, tal_topk 0.000,
tal_owner 0.000, tal_target 0.467, tal_dense 0.294, tal_box 0.094, tal_scalars 0.030 (recorded in strict_tal.RECORDED)"""


@pytest.fixture(autouse=True, scope="module")
def _report():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    yield
    print("\n" + sc.report())


# ------------------------------------------------------------------------------------------------ the hand-worked case
def test_hand_worked_case():
    """One 32 x 32 image: anchors 0..15 are the 4 x 4 stride-8 points (4, 12, 20, 28)^2, 16..19 the stride-16 points (8, 24)^2,
    20 the stride-32 point (16, 16).  Every box side is one-hot at bin 1 (logit 200), so a predicted box is the anchor point
    +- one stride: 16 x 16, 32 x 32, 64 x 64.  Every class logit is 0 (s = 1/2).  topk = 8, alpha = 0.5, beta = 6.
    GT 0 = [1, 15]^2 (class 0, area 196) holds the points 0, 1, 4, 5 (IoU 121 / 331 each: an 11 x 11 overlap with a 16 x 16 box)
    and 16 (IoU 196 / 1024); five candidates < topk: it takes them all.
    GT 1 = [9, 31]^2 (class 1, area 484) holds 5, 6, 7, 9, 10, 11, 13, 14, 15, 19, 20 with IoU 256/484 (10), 484/1024 (19),
    176/564 (the edge points 6, 9, 11, 14), 121/619 (the corner points 5, 7, 13, 15), 484/4096 (20).  Its top 8: 10, 19, the
    four edge points, and of the four tied corner points the two with the lowest index, 5 and 7.
    Anchor 5 is contested: IoU 121/331 with GT 0 against 121/619 with GT 1, so GT 0 keeps it.
    t = align * mi / (ma + 1e-9) with align = sqrt(1/2) IoU^6: for GT 0 ma, mi come from the tied points, for GT 1 from anchor 10.
    CIoU: all boxes are squares, so v = 0 (to 1e-18) and ciou = IoU - rho^2 / c^2: 32/722 for the points of GT 0 at stride 8,
    0 for 16 and 10 (same centre), 32/2048 for 19, 64/1213 for an edge point, 128/1458 for the corner point.
    DFL: log-softmax is 0 at bin 1 and -200 elsewhere, so a side with target tv costs 200 (1 - max(0, 1 - |tv - 1|)); the means
    over the four sides are 100 (0, 1, 4, 5), 112.5 (16), 75 (10), 62.5 (19), 118.75 (edge points), 162.5 (7).
    BCE at logit 0 is ln 2 whatever the target: cls = 2 * 21 * ln 2 / tss."""
    anchors, strides = tr.make_anchors(32, 32)
    assert anchors.shape[1] == 21
    preds = torch.zeros(1, 66, 21)
    for side in range(4):
        preds[0, side * 16 + 1] = 200.0
    gts = [torch.tensor([[8.0, 8.0, 14.0, 14.0, 0.0], [20.0, 20.0, 22.0, 22.0, 1.0]])]
    asg, ref = tr.loss(preds, anchors, strides, gts, dict(topk=8))
    owner = [0, 0, -1, -1, 0, 0, 1, 1, -1, 1, 1, 1, -1, -1, 1, -1, 0, -1, -1, 1, -1]
    assert asg["owner"][0].tolist() == owner
    assert [q[0] for q in asg["lists"][0]] == [0, 1, 4, 5, 16] and [q[0] for q in asg["lists"][1]] == [10, 19, 6, 9, 11, 14, 5, 7]
    t_a, t_16, t_10, t_19, t_edge, t_7 = 0.36555870, 0.0075326805, 0.52892559, 0.26933909, 0.022306341, 0.0013477064
    t = [t_a, t_a, 0, 0, t_a, t_a, t_edge, t_7, 0, t_edge, t_10, t_edge, 0, 0, t_edge, 0, t_16, 0, 0, t_19, 0]
    assert torch.allclose(asg["t"][0], torch.tensor(t, dtype=F64), rtol=1e-6, atol=0)
    assert math.isclose(ref["tss"], 2.3586052, rel_tol=1e-6)
    total, box, cls, dfl = 147.16267, 0.61956072, 12.342965, 90.896319
    assert torch.allclose(ref["out"], torch.tensor([total, box, cls, dfl], dtype=F64), rtol=1e-6, atol=0)
    assert math.isclose(float(asg["ma"][1]), math.sqrt(0.5) * (256 / 484) ** 6, rel_tol=1e-6) and math.isclose(float(asg["mi"][0]), 121 / 331, rel_tol=1e-6)


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("seed", range(4))
def test_invariants_of_the_reference_on_random_cases(seed):
    case = st.make_case(3, 96, 4, F32, seed=seed, built=False, fill=5, hyper=dict(topk=(10, 13, 3, 1)[seed]))
    asg, ref = st.reference(case)
    p, an, s_ = case.f(F64)
    gt, img = case.gt.to(F64), case.img
    k = case.hyper["topk"]
    claimed = torch.zeros(case.N, case.A, dtype=torch.long)
    for j, lst in enumerate(asg["lists"]):
        n = int(img[j])
        assert len(lst) <= k and len({q[0] for q in lst}) == len(lst)
        own = (asg["owner"][n] == j).nonzero().flatten().tolist()
        assert len(own) <= k and set(own) <= {q[0] for q in lst}                 # a GT owns at most topk anchors, all from its list
        claimed[n, own] += 1
        d = tr.inside(gt[j], an, s_)
        assert all(float(d[a_]) > tr.EPS9 for a_ in own)                          # every positive lies strictly inside its GT
        for a_ in own:
            assert 0.0 <= float(asg["t"][n, a_]) <= float(asg["mi"][j])          # 0 <= t <= mi
            assert int(asg["label"][n, a_]) == int(gt[j, 4])
    assert int(claimed.max()) <= 1 and torch.equal(claimed > 0, asg["owner"] >= 0)     # at most one owner per anchor
    assert ref["tss"] >= 1.0 and bool(torch.isfinite(ref["out"]).all()) and bool(torch.isfinite(ref["dp"]).all())
    assert not bool(ref["dp"][:, :64][(asg["label"] < 0)[:, None, :].expand(-1, 64, -1)].any())


def test_no_gt_at_all_leaves_bce_at_target_zero():
    case = st.make_case(2, 64, 4, F32, empty=(0, 1), built=False)
    asg, ref = st.reference(case)
    x = case.preds.double()[:, 64:]
    want = tr.bce(x, torch.zeros_like(x)).sum()
    assert ref["tss"] == 1.0 and float(ref["out"][1]) == 0.0 == float(ref["out"][3])
    assert torch.allclose(ref["out"][2], want) and torch.allclose(ref["out"][0], 0.5 * want)


# ------------------------------------------------------------------------------------------------ the stand-in passes
SHAPES = [(1, 64, 1, F32, {}), (3, 96, 4, BF, dict(hyper=dict(topk=13))), (3, 64, 80, HF, dict(empty=(1,))), (1, 96, 80, F32, {}),
          (3, 64, 4, HF, dict(grad_scale=65536.0)), (3, 96, 4, BF, dict(grad_scale=1024.0, empty=(0,)))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-w{s[1]}-nc{s[2]}-{str(s[3])[6:]}-{'-'.join(s[4]) or 'plain'}")
def test_stand_in_has_nothing_outside(shape):
    n, w, nc, dtype, kw = shape
    case = st.make_case(n, w, nc, dtype, **kw)
    assert case.redraws <= 1
    state = st.stand_in(case)
    st.verify(case, state)
    ref, ev = st.reference_terms(case, state), st.evaluate(case, state)
    # the analytic gradient the limits are propagated through IS the autograd gradient
    assert torch.allclose(ev["dp"], ref["dp"], rtol=1e-9, atol=1e-13) and torch.allclose(ev["out"], ref["out"], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ the comparator's proof
@pytest.fixture(scope="module")
def proof():
    case = st.make_case(3, 64, 4, F32, seed=1)
    state = st.stand_in(case)
    st.verify(case, state)
    return case, state, st.reference_terms(case, state), st.evaluate(case, state)


def _beyond(ref, noise):
    return (ref + 1.02 * (noise + sc.ulp(ref, F32))).float()


def _inside(ref, noise):
    return (ref + 0.98 * noise).float()


def _with(state, **kw):
    s = copy.copy(state)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("where", ["class", "class_of_a_positive", "box_of_a_positive", "box_of_no_positive"])
def test_a_gradient_just_beyond_its_limit_fails_and_one_just_inside_passes(proof, where):
    case, state, ref, ev = proof
    n, a = [int(v) for v in ev["pos"][0]]
    free = int((state.label[n] == -1).nonzero()[0])
    ch, an, fam = {"class": (64 + 1, free, "tal_dense"), "class_of_a_positive": (64 + int(state.label[n, a]), a, "tal_dense"),
                   "box_of_a_positive": (17, a, "tal_box"), "box_of_no_positive": (17, free, "tal_dense")}[where]
    r, nz = ref["dp"][n, ch, an], ev["dp_noise"][n, ch, an]
    bad, ok = state.dp.clone(), state.dp.clone()
    bad[n, ch, an], ok[n, ch, an] = _beyond(r, nz), _inside(r, nz)
    assert st.failing_families(lambda: st.check_values(case, _with(state, dp=bad))) == [fam]
    assert st.failing_families(lambda: st.check_values(case, _with(state, dp=ok))) == []
    if where == "box_of_no_positive":                         # exact zero: the smallest subnormal already fails
        assert float(r) == 0.0 and float(nz) == 0.0


@pytest.mark.parametrize("k", range(5))
def test_a_scalar_just_beyond_its_limit_fails_and_one_just_inside_passes(proof, k):
    case, state, ref, ev = proof
    if k < 4:
        r, nz = ref["out"][k], ev["out_noise"][k]
        bad, ok = state.out.clone(), state.out.clone()
        bad[k], ok[k] = _beyond(r, nz), _inside(r, nz)
        sb, so = _with(state, out=bad), _with(state, out=ok)
    else:
        r, nz = torch.tensor(ref["tss"], dtype=F64), ev["tss_noise"]
        sb, so = _with(state, tss=float(_beyond(r, nz))), _with(state, tss=float(_inside(r, nz)))
    assert st.failing_families(lambda: st.check_values(case, sb, families=("tal_scalars",))) == ["tal_scalars"]
    assert st.failing_families(lambda: st.check_values(case, so, families=("tal_scalars",))) == []


def test_a_target_just_beyond_its_limit_fails_and_one_just_inside_passes(proof):
    case, state, ref, ev = proof
    n, a = [int(v) for v in ev["pos"][0]]
    j = int(state.owner[n, a])
    al = next(q[1] for q in state.lists[j] if q[0] == a)
    t64 = al * float(state.mi[j]) / (float(state.ma[j]) + tr.EPS9)
    noise = torch.tensor(3.0 * st.U * t64, dtype=F64)
    for name, idx in (("t", (n, a)), ("ma", j), ("mi", j)):
        r, nz = (torch.tensor(t64, dtype=F64), noise) if name == "t" else (getattr(state, name)[idx].double(), torch.zeros((), dtype=F64))
        bad, ok = getattr(state, name).clone(), getattr(state, name).clone()
        bad[idx], ok[idx] = _beyond(r, nz), _inside(r, nz)
        assert st.failing_families(lambda: st.check_target(case, _with(state, **{name: bad}))) == ["tal_target"], name
        assert st.failing_families(lambda: st.check_target(case, _with(state, **{name: ok}))) == [], name


def test_a_chosen_set_with_one_wrong_member_fails(proof):
    case, state, _, _ = proof
    asg, _ = st.reference(case)
    j = next(j for j, c in enumerate(asg["cand"]) if case.hyper["topk"] + 2 < int(c.sum()) < case.A)
    chosen = {q[0] for q in state.lists[j]}
    al = asg["align"][j]
    out = [int(a) for a in asg["cand"][j].nonzero().flatten() if int(a) not in chosen]
    worst = min(out, key=lambda a: float(al[a]))                # the candidate with the smallest metric, far below the k-th
    n = int(case.img[j])
    row = case.gt[j].double()
    p, an, s_ = case.f(F64)
    _, a64, i64 = tr.metrics(state.pbox.double()[n], p[n, 64 + int(row[4])], row, an, s_, case.hyper["alpha"], case.hyper["beta"])
    lists = [list(l) for l in state.lists]
    lists[j][-1] = (worst, float(a64[worst].float()), float(i64[worst].float()))
    lists[j].sort(key=lambda q: (-q[1], q[0]))
    assert "tal_topk" in st.failing_families(lambda: st.check_topk(case, _with(state, lists=lists)))
    assert st.failing_families(lambda: st.check_topk(case, state)) == []
    # a non-candidate, a repeated anchor and a short list fail too
    for wrong in ([(q if i else (int((~asg["cand"][j]).nonzero()[0]), q[1], q[2])) for i, q in enumerate(state.lists[j])],
                  [state.lists[j][0]] + state.lists[j][:-1], state.lists[j][:-1]):
        lists = [list(l) for l in state.lists]
        lists[j] = wrong
        assert "tal_topk" in st.failing_families(lambda: st.check_topk(case, _with(state, lists=lists)))


def test_a_wrong_owner_fails(proof):
    case, state, _, _ = proof
    i, r1, r2 = case.props["twins"]
    off = sum(g.shape[0] for g in case.gts[:i])
    owner = state.owner.clone()
    owner[i][owner[i] == off + r1] = off + r2                   # the higher of two identical rows
    assert "tal_owner" in st.failing_families(lambda: st.check_owner(case, _with(state, owner=owner)))
    assert st.failing_families(lambda: st.check_owner(case, state)) == []


def test_redraw_cap_is_asserted(monkeypatch):
    calls = []
    monkeypatch.setattr(st, "guard_ok", lambda case, asg=None: calls.append(1) or len(calls) > 2)
    with pytest.raises(AssertionError, match="more than one in four"):
        st.make_case(1, 64, 1, F32, built=False)


# ------------------------------------------------------------------------------------------------ constructor and config
def test_constructor_refusals_and_defaults():
    from src.model.losses import YoloTALoss
    crit = YoloTALoss(num_classes=80)
    assert (crit.topk, crit.alpha, crit.beta, crit.lambda_box, crit.lambda_cls, crit.lambda_dfl) == (10, 0.5, 6.0, 7.5, 0.5, 1.5)
    assert YoloTALoss(num_classes=80, topk=13).topk == 13
    for bad in (dict(topk=0), dict(topk=17), dict(topk=2.5), dict(reg_max=8), dict(alpha=-1.0), dict(beta=float("nan"))):
        with pytest.raises(ValueError):
            YoloTALoss(num_classes=80, **bad)


def _script():
    path = os.path.join(ROOT, "custom-yolo-implmentation_amd", "scripts", "distributed_training.py")
    spec = importlib.util.spec_from_file_location("distributed_training_under_test_tal", path)
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def test_script_builds_the_criterion_from_training_loss():
    from src.model.losses import YoloDFLQFLoss, YoloTALoss
    script = _script()
    weights = {"weights": {"cls_loss": 2.0, "bbox_loss": 3.0}}
    for cfg in (weights, dict(weights, loss={"assigner": "nearest"})):             # absent / "nearest": today's arguments
        crit = script.build_criterion(cfg, 80)
        assert type(crit) is YoloDFLQFLoss and (crit.num_classes, crit.lambda_box, crit.lambda_cls, crit.lambda_dfl) == (80, 3.0, 2.0, 1.5)
    crit = script.build_criterion({"weights": {}}, 7)
    assert type(crit) is YoloDFLQFLoss and (crit.lambda_box, crit.lambda_cls) == (1.5, 1.0)
    crit = script.build_criterion(dict(weights, loss={"assigner": "tal"}), 80)
    assert type(crit) is YoloTALoss and (crit.num_classes, crit.topk, crit.alpha, crit.beta, crit.lambda_box, crit.lambda_cls,
                                         crit.lambda_dfl) == (80, 10, 0.5, 6.0, 7.5, 0.5, 1.5)
    crit = script.build_criterion(dict(weights, loss=dict(assigner="tal", topk=13, alpha=1.0, beta=4.0, box=5.0, cls=1.0, dfl=2.0)), 3)
    assert (crit.num_classes, crit.topk, crit.alpha, crit.beta, crit.lambda_box, crit.lambda_cls, crit.lambda_dfl) == (3, 13, 1.0, 4.0, 5.0, 1.0, 2.0)
    for bad in ({"assigner": "tal", "top_k": 10}, {"assigner": "atss"}, {"assigner": "nearest", "topk": 10}, {"assigner": "tal", "topk": 40},
                "tal"):
        with pytest.raises(ValueError):
            script.build_criterion(dict(weights, loss=bad), 80)
    import inspect
    assert "build_criterion(tr_cfg" in inspect.getsource(script.main)
    from src.utils.config_loader import load_config
    cfg = load_config(os.path.join(ROOT, "custom-yolo-implmentation_amd", "config.yaml"))
    assert "loss" not in cfg["training"] and type(script.build_criterion(cfg["training"], 80)) is YoloDFLQFLoss
    text = open(os.path.join(ROOT, "custom-yolo-implmentation_amd", "config.yaml")).read()
    assert '# loss: {assigner: "tal"' in text


def test_header_and_build_name_the_new_entry_points():
    from src.hipops import lib
    protos = lib.parse_header()
    assert "yolo_loss_tal" in protos and "yolo_loss_tal_workspace_bytes" in protos and "yolo_loss_dfl_qfl" in protos
    names = protos["yolo_loss_tal"][2]
    assert names[-1] == "st" and {"topk", "alpha", "beta", "lambda_box", "lambda_cls", "lambda_dfl", "grad_scale"} <= set(names)
    build = open(os.path.join(ROOT, "custom-yolo-implmentation_amd", "build.py")).read()
    assert '"loss_tal.hip"' in build.split("NO_CONTRACT", 2)[1].split("\n")[0]


def test_lazy_dict_carries_dfl_loss_only_with_four_scalars():
    from src.model.losses import LazyLossDict
    d3, d4 = LazyLossDict(torch.tensor([1.0, 2.0, 3.0])), LazyLossDict(torch.tensor([1.0, 2.0, 3.0, 4.0]))
    assert list(d3.keys()) == ["total_loss", "box_loss", "cls_loss"] and len(d3) == 3 and "dfl_loss" not in d3
    assert d4["dfl_loss"] == 4.0 and d4["box_loss"] == 2.0 and len(d4) == 4 and "dfl_loss" in d4
