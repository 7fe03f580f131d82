"""-m gpu: the kernels of csrc/decode_nms.hip held to tests/strict_post.py.  k_head_decode and k_dfl_expect inside the derived
per-element bound against float64 (class rows bit-equal); yolo_nms (k_cand_count, k_candidates, k_rank, k_mask, k_scan)
bit for bit against oracle.postproc.non_max_suppression: padded rows, counts and status; yolo_val_select (k_val_count,
k_val_candidates, k_val_rank, k_val_gather) against the decided sets of the float64 sigmoid; yolo_val_match (k_val_match)
counter for counter against the oracle's MetricCounters.  Every case runs twice and must repeat bit for bit.

Branches of decode_nms.hip and the case that reaches each (all compared with the oracle):
    img0 != 0 (second and third launch pair)   images: bs9-*, bs17-float32, bs17-max_det1 (images 8 and 16 differ from 0)
    rank >= MAX_NMS                            max_nms: 30208 candidates, isolated boxes at ranks 29999 | 30000 | 30100 / 100
    n > cap (status 1) and n == cap            capacity: 2049x64-overflow, 2048x64-exact-capacity
    c += 256 second trip (more than 256 chunks) chunks: 65793-f16-258-chunks (candidates behind chunk 256, the last anchor)
    M % 256 != 0, M < 256, word boundaries     compaction: M 1 .. 513, counts 0 / 1 / 64 / 65 / 128 / 129
    n > top_k on both sides (k_val_rank)       select: survivors-7-top_k-7 (all), survivors-8-top_k-7 (ranked), top_k >= M
    m > 64 * VAL_MAX_T (status 1)              match: m1025-*, the 33-image batch; m1024 is the last size matched
    NaN class scores (cand_eval, val_eval)     nonfinite-* of both"""
import time

import pytest
import torch

import strict_compare as sc
import strict_post as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, HF = sp.F32, sp.BF, sp.HF
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]
WANT = {}                     # NMS expectations, computed once per case


def ops():
    from src.hipops import ops as o
    return o


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    t0 = time.time()
    yield
    print("\n" + sc.report() + "\n" + sp.report() + f"\n[strict_post] wall time of tests/test_gpu_post.py: {time.time() - t0:.1f} s")


def twice(once):
    """run the case twice: every tensor it returns bit-identical; -> the first result"""
    a, b = once(), once()
    for x, y in zip(a, b):
        assert torch.equal(sp.bits(x), sp.bits(y)), "two runs differ"
    return a


def cpu(*ts):
    torch.cuda.synchronize()
    return tuple(t.detach().cpu() for t in ts)


# ------------------------------------------------------------------------------------------ decode, DFL
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("a,n,nc", sp.DECODE_CASES + [(25600, 1, 1)], ids=lambda v: str(v))
def test_head_decode_and_dfl_expect(a, n, nc, dtype):
    o = ops()
    p, anc, st, _ = sp.decode_case(a, n, nc, dtype)
    pd, ad, sd = p.to(DEV), anc.to(DEV), st.to(DEV)
    y, e = twice(lambda: cpu(o.head_decode(pd, ad, sd, nc), o.dfl_expect(pd[:, :64])))
    what = f"A={a} N={n} nc={nc} {IDS[DTYPES.index(dtype)]}"
    sp.check_decode(p, anc, st, nc, y, "head_decode " + what)
    sp.check_dfl(p[:, :64], e, "dfl_expect " + what)


# ------------------------------------------------------------------------------------------ NMS
def run_nms(case):
    o = ops()
    yd = case.y.to(DEV)
    return twice(lambda: cpu(*o.nms(yd, *case.args())))


def nms_want(case):
    if case.name not in WANT:
        WANT[case.name] = sp.nms_expect(case)
    return WANT[case.name]


@pytest.mark.parametrize("group", [g for g in sp.NMS_GROUPS if g != "capacity"])
def test_nms_rows_counts_and_status_are_the_oracles(group):
    for case in sp.nms_cases(group):
        rows, counts, status = run_nms(case)
        sp.check_nms(case, rows, counts, status, want=nms_want(case))


def test_nms_exact_capacity_and_overflow():
    from src.utils.model_utils import non_max_suppression
    exact, over = sp.nms_cases("capacity")
    rows, counts, status = run_nms(exact)
    sp.check_nms(exact, rows, counts, status, want=nms_want(exact))
    assert int(status[0]) == 0
    rows, counts, status = run_nms(over)
    sp.check_nms(over, rows, counts, status, want=nms_want(over))
    assert int(status[0]) == 1
    k = over.kw
    with pytest.raises(RuntimeError, match="capacity"):
        non_max_suppression(over.y.to(DEV), k["conf_thres"], k["iou_thres"], None, False, True, (), k["max_det"], over.nc)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nms_known_answers_through_the_wrapper(dtype):
    """the hand-computed keep lists of tests/test_nms_known.py (and the class-offset and 1/64-square cases of strict_post.KNOWN)
    on the device: boxes as xywh columns at dyadic coordinates, scores as one class"""
    from src.utils.model_utils import non_max_suppression
    for case in sp.known_cases(dtype):
        k = case.kw
        yd = case.y.to(DEV)
        got = twice(lambda: cpu(*non_max_suppression(yd, k["conf_thres"], k["iou_thres"], k["classes"], k["agnostic"], k["multi_label"],
                                                     (), k["max_det"], case.nc)))
        rows, counts, _ = sp.known_rows(case)
        assert len(got) == 1 and got[0].shape == (int(counts[0]), 6), (case.name, got[0].shape, int(counts[0]))
        sp.assert_exact(got[0], rows[0, :int(counts[0])], f"nms {case.name} (wrapper)", "post_nms", ("row", "column"))
        sp.check_nms(case, *cpu(*ops().nms(yd, *case.args())), want=(rows, counts, 0))


# ------------------------------------------------------------------------------------------ validation: select
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_val_select_decided_sets(dtype):
    o = ops()
    for case in sp.select_cases(dtype):
        yd = case.y.to(DEV)
        rows, count = twice(lambda: cpu(*o.val_select(yd, case.nc, case.conf, case.top_k)))
        sp.check_select(case, rows, count)


# ------------------------------------------------------------------------------------------ validation: match
def test_val_match_counters_are_the_oracles():
    o = ops()
    for case in sp.match_cases():
        rows, count, gt, off = case.rows.to(DEV), case.count.to(DEV), case.gt.to(DEV), case.off.to(DEV)
        if gt.numel() == 0:
            gt = torch.zeros(1, 5, device=DEV)                # a valid pointer for the image list without a target

        def once():
            ctr, status = case.start.clone().to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            o.val_match(rows, count, gt, off, case.thr, case.nc, case.skip, ctr, status)
            return cpu(ctr, status)

        ctr, status = twice(once)
        sp.check_match(case, ctr, status)
