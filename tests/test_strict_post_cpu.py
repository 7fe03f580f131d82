"""CPU tests of tests/strict_post.py: what proves, without a GPU, that the comparators of the decode, NMS and validation
kernels pass honest arithmetic and fail arithmetic that is subtly wrong, on the very cases tests/test_gpu_post.py runs.

References: decode_ref / dfl_ref are pinned to oracle.postproc.inference_decode (in float64) and to the reference's own
outputs in tests/golden/decode_val.npz and block_dfl.npz; nms_expect and nms_emul to tests/golden/nms.npz (six option sets);
match_emul to tests/golden/metrics.npz; the known-answer rows to the oracle.
Stand-ins with NOTHING outside any limit: tests/emulated_ops.py (head_decode, dfl_expect, nms, val_select, val_match) and
strict_post's own restatements of the kernels (decode_emul, dfl_emul, nms_emul, select_emul, match_emul) without a mutation.
Every case's undecided share of val_select from the reference alone is at most 0.5 %.
Every mutant of MUTANTS raises StrictMismatch in the family named beside it, on the named case of the GPU module's list.

Recorded maxima of the stand-ins (the module prints the table, run with -s): STAND_IN_MAXIMA."""
import pytest
import torch

import emulated_ops as emu
import strict_compare as sc
import strict_post as sp
from conftest import load_golden

F32, BF, HF = sp.F32, sp.BF, sp.HF
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]
STAND_IN_MAXIMA = """both stand-ins, every case of this module, 2026-10-20: post_decode 0.860, post_dfl 0.577 (of the noise, limit 1; the
same element as on the device: the subtraction a - E rounds alike wherever it is done in fp32); NMS, match: equal to the
oracle on every case; select: nothing outside, largest undecided share from the reference alone 0.0476 % (bf16), 0 (fp32, f16)"""


@pytest.fixture(autouse=True, scope="module")
def _threads_and_report():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    yield
    print("\n" + sc.report() + "\n" + sp.report())


def tid(d):
    return IDS[DTYPES.index(d)]


def nms_case(group, name):
    return next(c for c in sp.nms_cases(group) if c.name == name)


def sel_case(dtype, name):
    return next(c for c in sp.select_cases(dtype) if c.name.startswith(name))


def match_case(name):
    return next(c for c in sp.match_cases() if c.name == name)


# ------------------------------------------------------------------------------------------ the references are the oracle's
def test_the_decode_reference_is_the_oracle_and_the_golden():
    from oracle import postproc as opost
    from oracle.params import ParamStore
    p, anc, st, _ = sp.decode_case(257, 3, 8, F32)
    box, noise = sp.decode_ref(p, anc, st)
    ps = ParamStore()
    opost.inference_decode(ps, p[:1], anc, st, 8)             # creates the DFL weight (0 .. 15), kept in fp32
    for k in list(ps):
        ps[k] = ps[k].double()
    want = opost.inference_decode(ps, p.double(), anc.double(), st.double(), 8)
    assert float((box - want[:, :4]).abs().max()) <= 1e-10 and bool((noise > 0).all())
    gd = load_golden("decode_val")
    box, _ = sp.decode_ref(gd["preds"], gd["anchors"], gd["strides"])
    for i in range(2):
        for row in gd[f"out{i}"].reshape(-1, 5):
            d = (box[i] - row[:4].double().view(4, 1)).abs().amax(0)
            a = int(d.argmin())
            assert float(d[a]) <= 1e-4 and int(gd["preds"][i, 64:, a].argmax()) == int(row[4])
    g = load_golden("block_dfl")
    e, de = sp.dfl_ref(g["x"].double().view(3, 4, 16, 50))
    assert float((e - g["y"].double()).abs().max()) <= 5e-6            # the golden is an fp32 result at magnitudes up to 15


@pytest.mark.parametrize("tag,kw", [
    ("default", dict(conf_thres=0.25, iou_thres=0.45)), ("agnostic", dict(conf_thres=0.25, iou_thres=0.45, agnostic=True)),
    ("multi", dict(conf_thres=0.6, iou_thres=0.5, multi_label=True)), ("classes", dict(conf_thres=0.25, iou_thres=0.45, classes=[1, 3, 6])),
    ("maxdet", dict(conf_thres=0.25, iou_thres=0.9, max_det=17)), ("highconf", dict(conf_thres=0.999, iou_thres=0.45))])
def test_the_nms_references_are_the_golden(tag, kw):
    gd = load_golden("nms")
    case = sp.NmsCase(tag, gd["prediction"], 8, **kw)
    rows, counts, status = sp.nms_expect(case)
    for i in range(2):
        want = gd[f"{tag}:{i}"]
        want = want.reshape(-1, 6) if isinstance(want, torch.Tensor) else torch.zeros(0, 6)
        assert int(counts[i]) == want.shape[0] and torch.equal(rows[i, :want.shape[0]], want)
    sp.check_nms(case, *sp.nms_emul(case.y, *case.args()), want=(rows, counts, status))


def test_the_match_reference_is_the_golden():
    gd = load_golden("metrics")
    nc = int(gd["num_classes"])
    po, go = gd["pred_off"], gd["gt_off"]
    n = len(po) - 1
    k = int((po[1:] - po[:-1]).max())
    rows, count = torch.zeros(n, k, 6), torch.zeros(n, dtype=torch.int32)
    for i in range(n):
        c = int(po[i + 1] - po[i])
        rows[i, :c, :5], count[i] = gd["pred"][po[i]:po[i + 1]], c
    for thr in (0.5, 0.45):
        for fn in (emu.val_match, sp.match_emul):
            ctr = torch.zeros(5 + 4 * nc, dtype=torch.int64)
            fn(rows, count, gd["gt"], go.to(torch.int32), thr, nc, False, ctr, None)
            assert ctr[:5].tolist() == gd[f"thr{thr}:scalars_after_each"][-1].tolist()
            for j, name in enumerate(("class_tp", "class_fp", "class_fn", "class_gt")):
                assert ctr[5 + j * nc:5 + (j + 1) * nc].tolist() == gd[f"thr{thr}:{name}"].long().tolist(), name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_known_answers_are_the_oracles(dtype):
    for case in sp.known_cases(dtype):
        sp.check_nms(case, *sp.known_rows(case))              # the hand-computed keep lists against the oracle
        sp.check_nms(case, *sp.nms_emul(case.y, *case.args()))


# ------------------------------------------------------------------------------------------ the stand-ins
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("a,n,nc", sp.DECODE_CASES + [(25600, 1, 1)], ids=lambda v: str(v))
def test_decode_stand_ins_have_nothing_outside(a, n, nc, dtype):
    p, anc, st, take = sp.decode_case(a, n, nc, dtype)
    for name, got in (("emulated_ops", emu.head_decode(p, anc, st, nc)), ("decode_emul", sp.decode_emul(p, anc, st, nc))):
        sp.check_decode(p, anc, st, nc, got, f"{name} A={a} N={n} nc={nc} {tid(dtype)}")
    for name, got in (("emulated_ops", emu.dfl_expect(p[:, :64])), ("dfl_emul", sp.dfl_emul(p[:, :64]))):
        sp.check_dfl(p[:, :64], got, f"{name} A={a} N={n} {tid(dtype)}")


@pytest.mark.parametrize("group", sp.NMS_GROUPS)
def test_nms_stand_in_is_the_oracle(group):
    for case in sp.nms_cases(group):
        want = sp.nms_expect(case)
        rows, counts, status = sp.nms_emul(case.y, *case.args())
        sp.check_nms(case, rows, counts, status, want=want)
        if status == 0:
            assert float(rows[torch.arange(rows.shape[1]).view(1, -1) >= counts.view(-1, 1)].abs().sum()) == 0.0
    if group == "max_nms":                                    # what the two cases are built for
        a, b = sp.nms_cases(group)
        ra, rb = sp.nms_expect(a)[0][0], sp.nms_expect(b)[0][0]
        xs = lambda r: set(r[:, 0].tolist())
        assert 996.0 in xs(ra) and 1096.0 not in xs(ra) and 1196.0 not in xs(ra) and 1196.0 in xs(rb)
    if group == "capacity":
        assert sp.nms_expect(sp.nms_cases(group)[1])[2] == 1 and sp.nms_expect(sp.nms_cases(group)[0])[2] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_select_stand_ins_and_the_undecided_share_of_the_inputs(dtype):
    worst = 0.0
    for case in sp.select_cases(dtype):
        share = sp.select_undecided(case)
        assert share <= sp.UNDECIDED_CAP, (case.name, share)
        worst = max(worst, share)
        sp.check_select(case, *emu.val_select(case.y, case.nc, case.conf, case.top_k))
        sp.check_select(case, *sp.select_emul(case.y, case.nc, case.conf, case.top_k))
    print(f"\n[strict_post] {tid(dtype)}: largest undecided share from the reference alone {100 * worst:.4f} %")


def test_select_cases_reach_both_sides_of_the_switch():
    for dtype in DTYPES:
        counts = {c.name: emu.val_select(c.y, c.nc, c.conf, c.top_k)[1].tolist() for c in sp.select_cases(dtype)}
        assert counts["survivors-7-top_k-7"] == [7, 3] and counts["survivors-8-top_k-7"] == [7, 3]
        st = sp.sel_sets(sel_case(dtype, "survivors-8").y, 3, 0.5)
        assert int(st["must"][0].sum()) == 8 and int(st["maybe"][0].sum()) == 8
        rows, cnt = emu.val_select(sel_case(dtype, "equal-logits").y, 2, 0.5, 7)
        assert (rows[0, :, 0] + 128 * rows[0, :, 1]).tolist() == [10., 300., 511., 5., 20., 255., 256.]
        if dtype == F32:
            continue
        rows, cnt = emu.val_select(sel_case(dtype, "logit0").y, 2, 0.5, 100)
        assert cnt.tolist() == [3] and rows[0, :3, 5].tolist() == [0.5] * 3 and rows[0, :3, 4].tolist() == [0., 0., 0.]


def test_match_stand_in_is_the_oracle():
    for case in sp.match_cases():
        want = sp.match_expect(case)
        got = sp.match_expect(case, fn=sp.match_emul)
        sp.check_match(case, got[0], got[1], want=want)
    assert sp.match_expect(match_case("m1025-n12-skip0"))[1] == 1
    tie = sp.match_expect(match_case("tie-3-67"))[0]
    assert tie[:5].tolist() == [2, 70, 1, 1, 69]              # the lower index won: prediction 1 found it taken


# ------------------------------------------------------------------------------------------ the mutants
def _decode_mutant(mut, a, dtype):
    p, anc, st, take = sp.decode_case(a, 3, 8, dtype)
    fam = sp.failing_families(lambda: sp.check_decode(p, anc, st, 8, sp.decode_emul(p, anc, st, 8, mut, take), f"mutant {mut}"))
    if mut in ("bins1", "no_max"):
        fam += sp.failing_families(lambda: sp.check_dfl(p[:, :64], sp.dfl_emul(p[:, :64], mut), f"mutant {mut}"))
    return fam


def _nms_mutant(mut, group, name):
    case = nms_case(group, name) if group != "known" else next(c for d in DTYPES for c in sp.known_cases(d) if c.name == name)
    return sp.failing_families(lambda: sp.check_nms(case, *sp.nms_emul(case.y, *case.args(), mut=mut)))


def _select_mutant(mut, dtype, name):
    case = sel_case(dtype, name)
    return sp.failing_families(lambda: sp.check_select(case, *sp.select_emul(case.y, case.nc, case.conf, case.top_k, mut)))


def _match_mutant(mut, name):
    case = match_case(name)
    got = sp.match_expect(case, fn=lambda *a: sp.match_emul(*a, mut=mut))
    return sp.failing_families(lambda: sp.check_match(case, got[0], got[1]))


MUTANTS = [
    ("post_decode", "bins 1..16", lambda: _decode_mutant("bins1", 257, F32)),
    ("post_dfl", "bins 1..16 (dfl)", lambda: _decode_mutant("bins1", 257, HF)),
    ("post_decode", "E rounded to bf16 before the corners", lambda: _decode_mutant("round_e", 2100, BF)),
    ("post_decode", "E rounded to f16 before the corners", lambda: _decode_mutant("round_e", 2100, HF)),
    ("post_decode", "softmax without the max subtraction", lambda: _decode_mutant("no_max", 256, F32)),
    ("post_dfl", "softmax without the max subtraction (dfl)", lambda: _decode_mutant("no_max", 256, BF)),
    ("post_decode", "the neighbouring level's stride at a level boundary", lambda: _decode_mutant("stride", 2100, F32)),
    ("post_decode", "the neighbouring level's stride, A = 255", lambda: _decode_mutant("stride", 255, BF)),
    ("post_nms", ">= for > (IoU 0.5 at thr 0.5)", lambda: _nms_mutant("ge", "known", "known-half.5")),
    ("post_nms", ">= for > (IoU fl(0.6))", lambda: _nms_mutant("ge", "known", "known-tiny.6")),
    ("post_nms", "an epsilon in the union", lambda: _nms_mutant("eps", "known", "known-tiny.6-")),
    ("post_nms", "higher index first on ties", lambda: _nms_mutant("tie_high", "ties", "bf16-20-levels")),
    ("post_nms", "higher index first on ties, at max_det", lambda: _nms_mutant("tie_high", "ties", "bf16-ties-straddle-max_det")),
    ("post_nms", "xywh -> xyxy in fp32 (bf16)", lambda: _nms_mutant("xyxy_f32", "images", "bs9-bfloat16")),
    ("post_nms", "xywh -> xyxy in fp32 (f16)", lambda: _nms_mutant("xyxy_f32", "chunks", "65793-f16-258-chunks")),
    ("post_nms", "fused multiply-add", lambda: _nms_mutant("fma", "fma", "fma-pair")),
    ("post_nms", "class offset 4096", lambda: _nms_mutant("off4096", "known", "known-offset-4096")),
    ("post_nms", "MAX_NMS cut off by one", lambda: _nms_mutant("cut", "max_nms", "30208-isolated-rank-30100-dropped")),
    ("post_nms", "a row written past max_det", lambda: _nms_mutant("past_max_det", "images", "bs17-max_det1")),
    ("post_nms", "a later chunk reads the mask of image i - 8 (bs 9)", lambda: _nms_mutant("mask_prev", "images", "bs9-float32")),
    ("post_nms", "a later chunk reads the mask of image i - 8 (bs 17)", lambda: _nms_mutant("mask_prev", "images", "bs17-float32")),
    ("post_nms", "a NaN score skipped", lambda: _nms_mutant("nan_skip", "nonfinite", "nonfinite-float32-multi0")),
    ("post_nms", "a NaN score skipped, multi_label", lambda: _nms_mutant("nan_skip", "nonfinite", "nonfinite-float16-multi1")),
    ("post_select", "> for >= at conf", lambda: _select_mutant("gt", BF, "logit0")),
    ("post_select", "conf not rounded to bf16", lambda: _select_mutant("conf_raw", BF, "conf")),
    ("post_select", "conf not rounded to f16", lambda: _select_mutant("conf_raw", HF, "conf")),
    ("post_select", "last maximum", lambda: _select_mutant("last_max", HF, "logit0")),
    ("post_select", "last maximum, 80 classes bf16", lambda: _select_mutant("last_max", BF, "M257-nc80-N1-k100")),
    ("post_select", "higher anchor first on ties", lambda: _select_mutant("tie_high", HF, "equal-logits")),
    ("post_select", "a NaN score skipped", lambda: _select_mutant("nan_skip", F32, "nonfinite-k100")),
    ("post_select", "a NaN score skipped, ranked", lambda: _select_mutant("nan_skip", BF, "nonfinite-k3")),
    ("post_match", "last index on a tie, one lane", lambda: _match_mutant("tie_last", "tie-3-67")),
    ("post_match", "last index on a tie, two lanes", lambda: _match_mutant("tie_last", "tie-5-70")),
    ("post_match", "threshold compared in float", lambda: _match_mutant("thr_float", "thr-next-double-miss")),
    ("post_match", "totals advanced on the n == 0 path", lambda: _match_mutant("totals_n0", "m1-n0-skip0")),
    ("post_match", "a matched target reused", lambda: _match_mutant("reuse", "m63-n12-skip0")),
    ("post_match", "class ids rounded", lambda: _match_mutant("cls_round", "class-ids-nonzero-start")),
]


@pytest.mark.parametrize("family,name,run", MUTANTS, ids=[m[1] for m in MUTANTS])
def test_mutant_fails_in_its_family(family, name, run):
    sp.GUARD = False                  # a mutant may leave the former limit too: that assertion is not the comparator's finding
    keep = ({k: list(v) for k, v in sc.OBSERVED.items()}, list(sp.UNDECIDED))     # the tables record the stand-ins alone
    try:
        fams = run()
    finally:
        sp.GUARD = True
        sc.OBSERVED.clear()
        sc.OBSERVED.update(keep[0])
        sp.UNDECIDED[:] = keep[1]
    assert family in fams, f"mutant '{name}' survived (families that failed: {fams})"


def test_round_e_fails_in_the_sizes():
    """E rounded to T first: the centre keeps (E_r - E_l) / 2 small, the size E_l + E_r loses the low bits"""
    p, anc, st, take = sp.decode_case(2100, 1, 1, BF)
    got = sp.decode_emul(p, anc, st, 1)
    got[:, 2:4] = sp.decode_emul(p, anc, st, 1, "round_e", take)[:, 2:4]      # the honest centres, the mutant's sizes
    keep = {k: list(v) for k, v in sc.OBSERVED.items()}
    sp.GUARD = False
    try:
        with pytest.raises(sp.StrictMismatch) as ei:
            sp.check_decode(p, anc, st, 1, got, "round_e")
    finally:
        sp.GUARD = True
        sc.OBSERVED.clear()
        sc.OBSERVED.update(keep)
    assert all(ix[1] in (2, 3) for ix, *_ in ei.value.worst)


def test_failure_messages_name_image_row_and_column():
    case = nms_case("images", "bs9-float32")
    rows, counts, status = sp.nms_emul(case.y, *case.args())
    rows[8, 2, 4] += 1.0
    with pytest.raises(sp.StrictMismatch, match=r"'image': 8, 'row': 2, 'column': 4"):
        sp.check_nms(case, rows, counts, status)
    sel = sel_case(F32, "M257-nc80-N3-k7")
    rows, cnt = sp.select_emul(sel.y, sel.nc, sel.conf, sel.top_k)
    rows[2, 1, 5] = 0.999
    with pytest.raises(sp.StrictMismatch, match=r"image 2 row 1 column 5"):
        sp.check_select(sel, rows, cnt)
    rows, cnt = sp.select_emul(sel.y, sel.nc, sel.conf, sel.top_k)
    rows[1, 3, 2] = -0.0                                      # image 1 has no survivor: every row is past the count
    with pytest.raises(sp.StrictMismatch, match=r"image 1 row 3 column 2"):
        sp.check_select(sel, rows, cnt)
