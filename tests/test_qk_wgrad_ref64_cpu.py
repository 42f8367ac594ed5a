"""The q_norm / k_norm weight-gradient kernels (tasu_qk_norm_wgrad, tasu_f32_qk_norm_wgrad) on the CPU: the float64 reference of
tests/qk_wgrad_ref64.py checked on the torch restatement of tests/qwen3_full_ft_ops.py -- the same cases, profiles and checks the
GPU file runs on the kernels --, three mutants that must leave the bound or miss the exact bits, and the two entry points in the
header, the binding and the library, with every argument rule refused before any launch."""
import os

import pytest
import torch

import qk_wgrad_ref64 as Q
from conftest import ROOT
from qwen3_full_ft_ops import QkWgradTorch

NAMES = ("tasu_qk_norm_wgrad", "tasu_f32_qk_norm_wgrad")
ERR_ARG = 1


@pytest.mark.parametrize("family", Q.FAMILIES)
@pytest.mark.parametrize("c", Q.CASES, ids=Q.case_id)
def test_restatement_against_float64(c, family):
    ops = QkWgradTorch()
    for acc in (False, True):
        d = Q.inputs(c, family, "exact")
        assert Q.exact(Q.run(ops, d, acc), Q.reference(d, acc)), ("exact", acc)
        d = Q.inputs(c, family, "general")
        assert Q.ratio(Q.run(ops, d, acc), Q.reference(d, acc)) <= 1.0, ("general", acc)


@pytest.mark.parametrize("mutant,family", [("swap", "bf16"), ("swap", "f32"), ("no-round", "bf16"), ("v", "bf16"), ("v", "f32")])
def test_mutants_are_seen(mutant, family):
    """dwq and dwk exchanged, the bf16 rounding of xn dropped (the bf16 family's own; integers times a power of two need no
    rounding, so the general profile sees it), the v block included: each leaves the bound or misses the exact bits on every shape
    with more than one row.  The dropped rounding is a random 2^-9 of each term, about sqrt(N) 2^-9 of a term in the sum, while
    the worst-case bound grows as N^2 2^-24 of one: the bound sees it while N^1.5 < 2^15, so it is asked of the shapes with at most
    1200 terms (ratios at the largest of them: 3.0 at 300 x 4, 1.04 at 300 x 16, 0.30 at 700 x 16 -- the last two not asserted)."""
    ops = QkWgradTorch()
    ops.mutant = mutant
    for c in Q.CASES:
        if c.M == 1 or (mutant == "no-round" and c.M * c.H > 1200):
            continue
        d = Q.inputs(c, family, "general")
        missed_bound = Q.ratio(Q.run(ops, d, False, again=False), Q.reference(d, False)) > 1.0
        d = Q.inputs(c, family, "exact")
        missed_bits = not Q.exact(Q.run(ops, d, False, again=False), Q.reference(d, False))
        assert missed_bound and (missed_bits or mutant == "no-round"), (c, missed_bound, missed_bits)


def test_header_binding_and_library_agree():
    from ps_slm_amd import _lib
    from ps_slm_amd.model import qk_norm_wgrad_missing
    from ps_slm_amd.ops import QK_WGRAD_SPLIT, HipOps
    txt = open(os.path.join(ROOT, "include", "tasu_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in txt and name in _lib.PROTOTYPES, name
    assert f"#define TASU_QK_WGRAD_SPLIT {QK_WGRAD_SPLIT}" in txt and QK_WGRAD_SPLIT == Q.SPLIT
    assert _lib.ABI_VERSION >= 27 and f"#define TASU_ABI_VERSION {_lib.ABI_VERSION}" in txt
    lib = _lib.load()
    assert lib.tasu_abi_version() == _lib.ABI_VERSION and all(hasattr(lib, n) for n in NAMES)
    assert callable(getattr(HipOps, "qk_norm_wgrad", None)) and callable(getattr(HipOps, "f32_qk_norm_wgrad", None))
    assert qk_norm_wgrad_missing(None) is None and qk_norm_wgrad_missing(None, "fp32") is None
    assert qk_norm_wgrad_missing(QkWgradTorch()) is None and qk_norm_wgrad_missing(object()) == "qk_norm_wgrad"
    assert qk_norm_wgrad_missing(object(), "fp32") == "f32_qk_norm_wgrad"


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_refuse_bad_arguments_before_any_launch(name):
    """host buffers: every call is refused before any launch, so no pointer is ever dereferenced"""
    from ps_slm_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16)
    p = buf.data_ptr()
    assert p % 16 == 0
    fn = getattr(lib, name)
    need = Q.WS_FLOATS
    unit_limit = 0x7fffffff // (16 if name == "tasu_qk_norm_wgrad" else 32)

    def call(dqkv=p, pre=p + 4096, rstd=p, dwq=p, dwk=p + 512, ws=p, ws_floats=need, M=2, H=2, G=1, acc=0):
        return fn(dqkv, pre, rstd, dwq, dwk, ws, ws_floats, M, H, G, acc, None)

    for arg in ("dqkv", "pre", "rstd", "dwq", "dwk", "ws"):
        assert call(**{arg: None}) == ERR_ARG, arg                  # NULL pointers
    for arg in ("dqkv", "pre", "ws"):
        assert call(**{arg: p + 4}) == ERR_ARG, arg                 # 16-byte operands off alignment
    for arg in ("rstd", "dwq", "dwk"):
        assert call(**{arg: p + 2}) == ERR_ARG, arg                 # fp32 operands off alignment
    assert call(H=3, G=2) == ERR_ARG                                # H % G
    assert call(M=0) == ERR_ARG and call(H=0) == ERR_ARG and call(G=0) == ERR_ARG and call(M=-1) == ERR_ARG
    assert call(M=unit_limit // 4 + 1) == ERR_ARG                   # M * (H + 2G) over the sibling kernels' unit limit
    assert call(ws_floats=need - 1) == ERR_ARG and call(ws_floats=0) == ERR_ARG
    assert call(pre=p) == ERR_ARG                                   # dqkv == pre
