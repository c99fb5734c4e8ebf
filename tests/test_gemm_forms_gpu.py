"""The fp32 MFMA GEMM (csrc/gemm.h) form by form: every kernel instantiation behind gemm_f32_launch, and the host policies of
the NCF tower around it (pick_splits / gemm_auto + slices_epilogue_kernel, gemm_fwd_blocked), through the test and diagnostic
entry rk_gemm_f32 -- which reports the form the dispatcher chose, so each case ASSERTS that it reached the kernel it is
aimed at -- against the oracle's k-ordered fmaf chain, bit for bit (tests/_gemm_forms.py: the comparison rules, the two
derived exceptions, the guard regions).  Forms are selected by shape, strides and alignment alone.

The shapes are the smallest at which a form can go wrong: sizes that are no multiple of the tile or the chunk, one element,
more than one tile, ldc > N, N % 4 != 0, operands off 16-byte alignment, uneven last K-slices, catalogues smaller than a tile
under the acc_init prefix, several tiles per workgroup."""
import numpy as np
import pytest
import torch

from recad_amd import _lib

from . import _gemm_forms as GF
from ._gemm_forms import (DEEP_11_32, DEEP_11_64, DEEP_12_32, DEEP_12_64, DEEP_22_32, DEEP_22_64, SKINNY, TILE128, TILE128_GATHER,
                          TILE128_GATHER_PLAIN, WIDE_11, WIDE_11_PLAIN, WIDE_11_PLAIN_GROUPED, WIDE_12)

pytestmark = pytest.mark.gpu

EPI = dict(col_bias=True, relu=True)                                   # the tower's forward epilogue
SCORE = dict(row_bias=True, col_bias=True, const_add=0.25)             # the scoring epilogue


def case(name, M, N, K, form, **kw):
    return pytest.param(M, N, K, dict(form=form, **kw), id=name)


CASES = [
    # ---- skinny, 32-deep chunks: M, N, K off the 64 / 64 / 4 grid, every operand layout, every epilogue
    case("skinny-1x1x1", 1, 1, 1, SKINNY),
    case("skinny-63x65x33-epi", 63, 65, 33, SKINNY, **EPI),
    case("skinny-63x65x33-dx-layout-score", 63, 65, 33, SKINNY, lb="r", **SCORE),
    case("skinny-64x64x32-full-tile", 64, 64, 32, SKINNY),
    case("skinny-64x64x64-dw-layout", 64, 64, 64, SKINNY, la="r", lb="r"),
    case("skinny-100x12x24-mask-ld", 100, 12, 24, SKINNY, mask=True, ldmask=17),
    case("skinny-100x12x24-dw-layout-sigmoid", 100, 12, 24, SKINNY, la="r", lb="r", sigmoid=True),
    case("skinny-130x6x12-ldc6", 130, 6, 12, SKINNY, ldc=6),
    case("skinny-130x6x12-ldc11-bias", 130, 6, 12, SKINNY, ldc=11, col_bias=True),
    case("skinny-1000x4x8-epi", 1000, 4, 8, SKINNY, **EPI),
    case("skinny-65x70x20-dropout", 65, 70, 20, SKINNY, keep_prob=0.75, col_bias=True),
    # operands one float off 16-byte alignment / row strides off the float4 grid: no vector loads, and the deep form is refused
    case("skinny-128x64x128-A-off1", 128, 64, 128, SKINNY, a_off=1, **EPI),
    case("skinny-128x64x128-B-off1-dx", 128, 64, 128, SKINNY, lb="r", b_off=1),
    case("skinny-128x64x128-rs-odd", 128, 64, 128, SKINNY, a_pad=1, b_pad=3),
    case("skinny-64x64x128-dw-cs-odd-C-off1", 64, 64, 128, SKINNY, la="r", lb="r", a_pad=2, c_off=1),
    # ---- skinny, split-K by atomics into a C that already holds a value
    case("skinny-atomics-40x72x1000-dw-8", 40, 72, 1000, SKINNY, la="r", lb="r", split_k=8, splits=8),
    case("skinny-atomics-64x64x640-3-uneven", 64, 64, 640, SKINNY, split_k=3, splits=3),
    case("skinny-atomics-30x20x50-ldc", 30, 20, 50, SKINNY, split_k=4, splits=2, ldc=23),
    case("skinny-split-one-chunk", 30, 20, 32, SKINNY, split_k=4, splits=1),
    # ---- skinny, parked slices
    case("skinny-parked-100x24x300-4", 100, 24, 300, SKINNY, split_k=4, splits=4, parked=True),
    case("skinny-parked-100x24x300-dx-ldc", 100, 24, 300, SKINNY, lb="r", split_k=4, splits=4, parked=True, ldc=29),
    # ---- deep (128-deep chunks), 32-row half tiles
    case("deep32-11-128x64x128-epi", 128, 64, 128, DEEP_11_32, **EPI),
    case("deep32-12-64x128x256-mask-ld", 64, 128, 256, DEEP_12_32, lb="r", mask=True, ldmask=133),
    case("deep32-22-64x64x512", 64, 64, 512, DEEP_22_32, la="r", lb="r"),
    case("deep32-11-64x64x256-score-ldc", 64, 64, 256, DEEP_11_32, ldc=70, **SCORE),
    case("deep32-22-128x128x128-pads", 128, 128, 128, DEEP_22_32, la="r", lb="r", a_pad=4, b_pad=8, **EPI),
    # ---- deep, 64-row tiles
    case("deep64-11-1024x1024x128-epi", 1024, 1024, 128, DEEP_11_64, **EPI),
    case("deep64-12-1024x1024x128-mask", 1024, 1024, 128, DEEP_12_64, lb="r", mask=True),
    case("deep64-22-1024x1024x128", 1024, 1024, 128, DEEP_22_64, la="r", lb="r"),
    case("deep64-11-256x256x2048-atomics-16", 256, 256, 2048, DEEP_11_64, split_k=16, splits=16),
    case("deep64-22-256x256x2048-parked-16", 256, 256, 2048, DEEP_22_64, la="r", lb="r", split_k=16, splits=16, parked=True),
    case("deep64-12-256x256x2048-parked-16", 256, 256, 2048, DEEP_12_64, lb="r", split_k=16, splits=16, parked=True),
    # ---- deep, uneven last slice: 36 chunks as 8, 8, 8, 8, 4
    case("deep32-11-64x128x1152-parked-5", 64, 128, 1152, DEEP_11_32, split_k=5, splits=5, parked=True),
    case("deep32-22-64x128x1152-atomics-5", 64, 128, 1152, DEEP_22_32, la="r", lb="r", split_k=5, splits=5),
    # ---- wide<1,1> general through a_ridx: partial tiles both ways, N % 4 != 0
    case("wide11-300x333x128-mask-relu-bias", 300, 333, 128, WIDE_11, ridx="perm", mask=True, ldmask=335, **EPI),
    case("wide11-200x130x64-score-sigmoid", 200, 130, 64, WIDE_11, ridx="perm", sigmoid=True, **SCORE),
    case("wide11-129x257x64-identity-bias", 129, 257, 64, WIDE_11, ridx="identity", col_bias=True, ldc=259),
    # ---- wide<1,1> continuing the acc_init prefix (the evaluation's layer 0 over the item half)
    case("wide11-acc-300x128-rmod100", 300, 128, 64, WIDE_11, rmod=100, roff=0, prefix_k=64, init_base=-2, **EPI),
    case("wide11-acc-300x130-rmod128-off37", 300, 130, 64, WIDE_11, rmod=128, roff=37, prefix_k=64, init_base=-1, **EPI),
    case("wide11-acc-420x257-rmod257-off37", 420, 257, 64, WIDE_11, rmod=257, roff=37, prefix_k=20, init_base=-3, **EPI),
    case("wide11-acc-300x130-rmod100-base2", 300, 130, 128, WIDE_11, rmod=100, roff=237, prefix_k=64, init_base=2),
    # ---- wide<1,2>: B row-contiguous (dX); the right strip goes to another kernel
    case("wide12-256x300x64-identity-mask", 256, 300, 64, WIDE_12, strip=TILE128_GATHER, lb="r", ridx="identity", mask=True),
    case("wide12-256x300x64-perm-mask", 256, 300, 64, WIDE_12, strip=TILE128_GATHER, lb="r", ridx="perm", mask=True, ldmask=301),
    case("wide12-300x256x128-perm-no-strip", 300, 256, 128, WIDE_12, lb="r", ridx="perm", **EPI),
    case("wide12-2048x3100x64-strip-skinny", 2048, 3100, 64, WIDE_12, strip=SKINNY, lb="r", mask=True),
    # ---- wide<1,1,PLAIN> and its GROUPED variant (rows of C on 128-byte lines)
    case("wideplain-300x257x64", 300, 257, 64, WIDE_11_PLAIN, ridx="perm"),
    case("wideplain-300x257x128-C-off4", 300, 257, 128, WIDE_11_PLAIN, ridx="perm", ldc=288, c_off=4),
    case("widegrouped-300x257x64-ldc288", 300, 257, 64, WIDE_11_PLAIN_GROUPED, ridx="perm", ldc=288),
    case("widegrouped-256x384x192", 256, 384, 192, WIDE_11_PLAIN_GROUPED, ridx="identity"),
    # ---- 128-tile, no gather
    case("tile128-2048x3072x33-epi", 2048, 3072, 33, TILE128, **EPI),
    case("tile128-2tiles-per-block-131073x130x32", 131073, 130, 32, TILE128, col_bias=True),
    # ---- 128-tile gather continuing the acc_init prefix: catalogues smaller than, equal to and larger than a tile, the chunk
    #      starting in the middle of a user
    case("tile128-acc-50x70-rmod5", 50, 70, 12, TILE128_GATHER, rmod=5, roff=3, prefix_k=12, init_base=-1, **EPI),
    case("tile128-acc-300x70-rmod5-base2", 300, 70, 12, TILE128_GATHER, rmod=5, roff=13, prefix_k=12, init_base=2, **EPI),
    case("tile128-acc-300x130-rmod127", 300, 130, 12, TILE128_GATHER, rmod=127, roff=100, prefix_k=12, init_base=-4, **EPI),
    case("tile128-acc-300x70-rmod128", 300, 70, 12, TILE128_GATHER, rmod=128, roff=1, prefix_k=12, init_base=-1, **EPI),
    case("tile128-acc-300x70-rmod129", 300, 70, 12, TILE128_GATHER, rmod=129, roff=128, prefix_k=12, init_base=-1),
    case("tile128-acc-50x33-rmod300", 50, 33, 12, TILE128_GATHER, rmod=300, roff=280, prefix_k=12, init_base=-7, **EPI),
    case("tile128-acc-300x70-rmod300", 300, 70, 12, TILE128_GATHER, rmod=300, roff=150, prefix_k=12, init_base=-1, **EPI),
    case("tile128-rmod-no-prefix", 200, 70, 20, TILE128_GATHER, rmod=33, roff=5),
    # ---- 128-tile gather: the dropout epilogue (MF scoring in training mode), the PLAIN instantiation
    case("tile128-gather-200x150x16-dropout", 200, 150, 16, TILE128_GATHER, ridx="perm", keep_prob=0.75, **SCORE),
    case("tile128-gather-300x130x40-dw-layout-mask", 300, 130, 40, TILE128_GATHER, ridx="perm", la="r", lb="r", mask=True),
    case("tile128-gatherplain-200x150x33", 200, 150, 33, TILE128_GATHER_PLAIN, ridx="perm"),
    case("tile128-gatherplain-1x1x1", 1, 1, 1, TILE128_GATHER_PLAIN, ridx="identity"),
    case("tile128-gatherplain-130x129x64-A-off1", 130, 129, 64, TILE128_GATHER_PLAIN, ridx="perm", a_off=1, ldc=131),
    # ---- policy 1, gemm_auto (NCF's dX): splits where whole-K would not fill the chip, not where the deep kernel applies,
    #      never without a workspace
    case("auto-1000x24x300-dx-splits", 1000, 24, 300, SKINNY, policy=1, lb="r", mask=True, scratch_floats=5 * 1000 * 24 + 64, splits=5, must_split=True),
    case("auto-1000x24x300-cap-3-slices", 1000, 24, 300, SKINNY, policy=1, lb="r", col_bias=True, relu=True, scratch_floats=3 * 1000 * 24 + 100,
         splits=3, must_split=True),
    case("auto-1024x512x256-whole-k", 1024, 512, 256, DEEP_12_32, policy=1, lb="r", mask=True, scratch_floats=1 << 20, splits=1),
    case("auto-1000x24x300-no-scratch", 1000, 24, 300, SKINNY, policy=1, lb="r", mask=True, scratch_floats=None, splits=1),
    case("auto-1000x22x300-n-odd", 1000, 22, 300, SKINNY, policy=1, lb="r", mask=True, scratch_floats=1 << 18, splits=1),
    # ---- policy 2, gemm_fwd_blocked (the blocked training forward)
    case("blocked-64x128x256", 64, 128, 256, SKINNY, policy=2, scratch_floats=8 * 64 * 128, splits=8, **EPI),
    case("blocked-1000x12x256-16-row-chunks", 1000, 12, 256, SKINNY, policy=2, scratch_floats=8 * 12 * 64 + 95, splits=8, **EPI),
    case("blocked-200x64x512-no-bias", 200, 64, 512, SKINNY, policy=2, scratch_floats=8 * 200 * 64, splits=8, relu=True),
]


@pytest.mark.parametrize("M,N,K,kw", CASES)
def test_gemm_form(gpu_device, M, N, K, kw):
    kw = dict(kw)
    must_split = kw.pop("must_split", False)
    form, strip, splits = GF.run_case(gpu_device, M, N, K, **kw)
    assert (form, strip) == (kw["form"], kw.get("strip", GF.NONE))
    if must_split:   # a shape meant to split must not pass by silently going whole-K
        assert splits > 1, splits


def test_every_form_is_asserted_somewhere():
    """Every instantiation behind gemm_f32_launch appears among the forms the cases above assert (as the launch or as the right
    strip's launch): a dispatcher change that makes a form unreachable fails its case, a new form without a case fails here."""
    asserted = set()
    for p in CASES:
        kw = p.values[3]
        asserted.add(kw["form"])
        asserted.add(kw.get("strip", GF.NONE))
    asserted.discard(GF.NONE)
    assert asserted == set(GF.ALL_FORMS), sorted(GF.name_of(f) for f in set(GF.ALL_FORMS) ^ asserted)
    assert len(_lib.RK_GEMM_FORMS) == max(GF.ALL_FORMS) + 2   # + "none" and the tuning builds' variant


def _desc(dev, M, N, K, over):
    """a well-formed k-contiguous request on zero-filled buffers (argument checks: nothing is compared)"""
    t = dict(A=torch.zeros(M * K, device=dev), B=torch.zeros(N * K, device=dev), C=torch.zeros(M * N, device=dev),
             v=torch.zeros(max(M, N) * max(N, 4), device=dev))
    d = _lib.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A, d.a_rs, d.a_cs, d.B, d.b_rs, d.b_cs, d.C, d.ldc = t["A"].data_ptr(), K, 1, t["B"].data_ptr(), K, 1, t["C"].data_ptr(), N
    for k, v in over.items():
        setattr(d, k, t["v"].data_ptr() if v == "ptr" else v)
    return d, t


def test_blocked_forward_scratch_too_small(gpu_device):
    """gemm_fwd_blocked with less than 8 * 64 * N floats of workspace (or none): RK_EINVAL with the documented message, C untouched."""
    M, N, K = 100, 12, 256
    for floats in (8 * 64 * N - 1, None):
        cbuf = GF.Guarded(gpu_device, M * N)
        scr = GF.Guarded(gpu_device, 8 * 64 * N)
        d, keep = _desc(gpu_device, M, N, K, dict(policy=2, relu=1))
        d.C = cbuf.ptr
        if floats is not None:
            d.scratch, d.scratch_floats = scr.ptr, floats
        rc, _, _, _ = GF.call(d)
        assert rc == GF.RK_EINVAL
        assert _lib.lib().rk_last_error().decode() == f"ncf: the blocked forward needs desc.gemm_scratch of >= {8 * 64 * N} floats"
        cbuf.read(), scr.read()
        assert cbuf.untouched(np.zeros(M * N, dtype=bool)) and scr.untouched(np.zeros(8 * 64 * N, dtype=bool))


@pytest.mark.parametrize("over", [dict(ldc=11), dict(mask="ptr", ldmask=11), dict(row_bias="ptr"), dict(acc_init="ptr", ld_init=12),
                                  dict(acc_init="ptr", a_rmod=5, ld_init=11), dict(acc_init="ptr", a_rmod=5, ld_init=12, init_base=1),
                                  dict(split_k=2, relu=1), dict(split_k=2, a_rmod=5), dict(split_k=2, sk_part="ptr", sk_stride=100),
                                  dict(policy=3), dict(policy=1, sigmoid=1), dict(policy=1, ldc=13), dict(policy=2, relu=0, scratch="ptr", scratch_floats=1 << 20),
                                  dict(policy=2, relu=1, K=100, a_rs=100, b_rs=100, scratch="ptr", scratch_floats=1 << 20), dict(M=0), dict(A=None)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_gemm_entry_refuses_what_the_kernels_take_on_trust(gpu_device, over):
    """rk_gemm_f32 is a public entry in front of kernels that trust their callers: a request that would index out of bounds, or
    that a policy does not take, is RK_EINVAL with nothing launched (C keeps its sentinel)."""
    M, N, K = 20, 12, 256
    cbuf = GF.Guarded(gpu_device, M * 13)
    d, keep = _desc(gpu_device, M, N, K, over)
    if "A" not in over:
        d.C = cbuf.ptr
    rc, _, _, _ = GF.call(d)
    assert rc == GF.RK_EINVAL, rc
    assert _lib.lib().rk_last_error().decode().startswith("rk_gemm_f32:")
    cbuf.read()
    assert cbuf.untouched(np.zeros(M * 13, dtype=bool))


def test_gemm_forms_randomised(gpu_device):
    """20 cases of the randomised sweep (tests/tools/gemm_forms_stress.py: M, N in [1, 400], K in [1, 300], the three operand
    layouts, epilogues, gathers, K-splits), compared by the same rules; the forms it reached include the two that small
    shapes land on."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "gemm_forms_stress.py")
    spec = importlib.util.spec_from_file_location("gemm_forms_stress", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    forms = mod.run(seed=1234, n_cases=20)
    assert {SKINNY, TILE128_GATHER} <= forms, sorted(GF.name_of(f) for f in forms)
