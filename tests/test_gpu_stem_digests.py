"""-m gpu: the three stem kernels of csrc/stem.hip (k_stem_conv, k_stem_wgrad, k_stem_bn_wgrad) share one tile decode, one tap
map, one pixel-run gather and one wave combine.  The tests that hold them to float64 compare that shared code
with a bound; this one holds it to the BYTES the kernels wrote before the pieces were shared: SHA-256 digests recorded on an
MI355X by tools/record_stem_digests.py from the commit named in tests/golden/stem_routes.json (the parent of the refactor,
never the code under test).

Per case the inputs are strict_stem_bwd.make_inputs from a fixed seed.  The forward runs without a statistics accumulator and
mean / invstd / scale / shift are formed on the host from y.cpu() with correctly rounded sums (math.fsum): the accumulator is
filled by float atomics, whose order is not fixed, and a digest must not depend on it.  Seven outputs per case: y of
stem_conv_fwd, y of its bias + SiLU form, dw of stem_wgrad in fp32 and bf16, dw / dgamma / dbeta of stem_bn_wgrad."""
import hashlib
import json
import math
import os

import pytest
import torch

import strict_bn as sb
import strict_stem_bwd as ss
from test_gpu_kernels import DEV, dev, nhwc, ops

BF16, F16 = torch.bfloat16, torch.float16
# N, H, W, Cout, dtype, act
CASES = [(2, 38, 264, 32, BF16, 1),       # 16-byte staging, OW = 132: the second segment has 4 live pixels and reads its left-edge
                                          # column from the image; OH = 19: a half-empty last row pair
         (2, 37, 261, 16, F16, 1),        # W % 4 != 0: the scalar staging path; odd H
         (1, 8, 8, 48, BF16, 0),          # one tile, nearly all padding
         (9, 464, 8, 16, BF16, 1)]        # 9 x 116 x 1 = 1044 tiles > STEM_WG_SLABS (1024) > STEM_BN_SLABS (512): both grid-stride
                                          # loops and the fetch of the next tile
CASES += [(1, 10, 272, c, BF16, 1) for c in (64, 96, 128)]      # the other channel-tile counts: 96 leaves four threads without a
                                                                 # chunk, 128 fills the LDS
IDS = [f"{n}x{h}x{w}c{c}-{'bf16' if t is BF16 else 'f16'}-{'silu' if a else 'id'}" for n, h, w, c, t, a in CASES]
OUTPUTS = ("y", "y_bias_silu", "wgrad_f32", "wgrad_bf16", "bn_dw", "bn_dgamma", "bn_dbeta")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stem_routes.json")
EPS = 1e-3


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _host_coefficients(y, gamma, beta):
    """mean, invstd, scale, shift (fp32) of y's channels: float64 on the host, every sum correctly rounded"""
    a = y.cpu().double().permute(1, 0, 2, 3).reshape(y.shape[1], -1)
    count = a.shape[1]
    m = torch.tensor([math.fsum(r) for r in a.tolist()], dtype=torch.float64) / count
    sq = torch.tensor([math.fsum(r) for r in (a * a).tolist()], dtype=torch.float64) / count       # a * a is exact in float64
    invstd = (((sq - m * m).clamp_min(0.0) + sb.f32_of(EPS)) ** -0.5).float()
    mean = m.float()
    scale = gamma.float() * invstd
    return mean, invstd, scale, beta.float() - mean * scale


def case_digests(i):
    """-> {output name: sha256 hex of its bytes} of CASES[i]"""
    n, h, w, cout, dtype, act = CASES[i]
    o = ops()
    img, wt, gamma, beta, dout = ss.make_inputs(n, h, w, cout, dtype, seed=40 + i)
    img_d, dout_d, gamma_d = img.to(DEV), dev(nhwc(dout)), gamma.to(DEV)
    wp = o.stem_pack_weights(wt.to(DEV), dtype)
    y = o.stem_conv_fwd(img_d, wp, cout, dtype, None)
    y_act = o.stem_conv_fwd(img_d, wp, cout, dtype, None, bias=beta.float().to(DEV), act=1)
    mean, invstd, scale, shift = (t.to(DEV) for t in _host_coefficients(y, gamma, beta))
    w32, w16 = o.stem_wgrad(img_d, dout_d, torch.float32), o.stem_wgrad(img_d, dout_d, BF16)
    dw, dgamma, dbeta = o.stem_bn_wgrad(img_d, dout_d, y, scale, shift, mean, invstd, gamma_d, act, torch.float32)
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS, map(_sha, (y, y_act, w32, w16, dw, dgamma, dbeta))))


def digests():
    """-> {"<case id>/<output>": sha256 hex}: what tools/record_stem_digests.py writes"""
    return {f"{IDS[i]}/{k}": v for i in range(len(CASES)) for k, v in case_digests(i).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_stem_outputs_reproduce_the_recorded_digests(i):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want["digests"]) == len(CASES) * len(OUTPUTS)
    got = case_digests(i)
    bad = sorted(k for k in OUTPUTS if got[k] != want["digests"][f"{IDS[i]}/{k}"])
    print(f"\n[digests] {IDS[i]}: {len(OUTPUTS) - len(bad)} of {len(OUTPUTS)} outputs equal those of commit {want['commit'][:7]}", end="")
    assert not bad, f"{IDS[i]}: outputs differ from those of commit {want['commit'][:7]}: {bad}"
