"""Host-side pieces of full fine-tuning on the fp32 training step (csrc/wgrad_f32.hip): the header and the ctypes table declare the
new entry points, the ABI version moved, and every broken argument rule is refused before any launch (no GPU needed: a refused call
dereferences nothing, so the operands are plain 16-byte aligned addresses)."""
import os
import re

from conftest import ROOT

NEW = ("tasu_f32_gemm_tn_split", "tasu_f32_gemm_tn", "tasu_f32_rmsnorm_wgrad", "tasu_f32_colsum_split")
A, B, C, W = 0x10000, 0x20000, 0x30000, 0x40000                      # never dereferenced


def test_header_and_prototypes_declare_the_entry_points_and_the_abi_grew():
    from ps_slm_amd import _lib
    txt = open(os.path.join(ROOT, "include", "tasu_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in _lib.PROTOTYPES
    assert "ps-slm.py:105-108" in txt and "deepspeed_utils.py:205-236" in txt     # the reference spans the kernels replace
    assert re.search(r"#define TASU_F32_GEMM_TN_MAX_SPLIT 16\b", txt)
    assert int(re.search(r"#define TASU_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION
    assert _lib.ABI_VERSION >= 22                                     # 21 before the fp32 weight gradients
    lib = _lib.load()
    assert lib.tasu_abi_version() == _lib.ABI_VERSION
    # the ctypes table's arity equals the declaration's
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", txt).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name]), name


def test_gemm_tn_split_is_host_code():
    from ps_slm_amd import _lib
    lib = _lib.load()
    assert lib.tasu_f32_gemm_tn_split(0, 64, 64) == -1 and lib.tasu_f32_gemm_tn_split(64, 0, 64) == -1
    assert lib.tasu_f32_gemm_tn_split(1, 4, 4) == 1                   # one 16-row stage: nothing to cut
    assert lib.tasu_f32_gemm_tn_split(4096, 64, 64) == 16             # the cap
    assert lib.tasu_f32_gemm_tn_split(40, 64, 64) == 3                # never more ranges than stages
    assert lib.tasu_f32_gemm_tn_split(4096, 1536, 1536) == 3          # o_proj at Qwen2.5-1.5B: 144 tiles
    assert lib.tasu_f32_gemm_tn_split(4096, 17920, 1536) == 1 and lib.tasu_f32_gemm_tn_split(4096, 151936, 1536) == 1


def test_gemm_tn_refuses_every_broken_rule_before_any_launch():
    from ps_slm_amd import _lib
    lib = _lib.load()

    def call(a=A, lda=136, b=B, ldb=72, c=C, ldc=72, R=128, N=128, K=64, acc=0, nsplit=1, w=None, wf=0):
        return lib.tasu_f32_gemm_tn(a, lda, b, ldb, c, ldc, R, N, K, acc, nsplit, w, wf, None)

    assert call(a=None) == 1 and call(b=None) == 1 and call(c=None) == 1
    assert call(R=0) == 1 and call(N=0) == 1 and call(K=0) == 1
    assert call(N=126) == 1 and call(K=62) == 1                       # N % 4, K % 4
    assert call(lda=124) == 1 and call(ldb=60) == 1 and call(ldc=60) == 1      # shorter than the operand (ldc < K)
    assert call(lda=138) == 1 and call(ldb=74) == 1 and call(ldc=74) == 1      # % 4
    assert call(a=A + 4) == 1 and call(b=B + 8) == 1 and call(c=C + 12) == 1   # 16-byte alignment
    assert call(nsplit=0) == 1 and call(nsplit=9) == 1 and call(nsplit=17, R=4096) == 1   # 128 rows = 8 stages; the cap
    assert call(nsplit=2) == 1                                        # a split without a workspace
    assert call(nsplit=2, w=W, wf=2 * 128 * 64 - 1) == 1 and call(nsplit=2, w=W + 4, wf=2 * 128 * 64) == 1


def test_rmsnorm_wgrad_and_colsum_split_refuse_every_broken_rule_before_any_launch():
    from ps_slm_amd import _lib
    lib = _lib.load()
    R, D, full = 8, 256, 64 * 256 + 8

    def rms(dy=A, x=B, rstd=None, dw=C, w=W, wf=full, R=R, D=D):
        return lib.tasu_f32_rmsnorm_wgrad(dy, x, rstd, dw, w, wf, R, D, 1e-6, 0, None)

    assert rms(dy=None) == 1 and rms(x=None) == 1 and rms(dw=None) == 1 and rms(w=None) == 1
    assert rms(R=0) == 1 and rms(D=0) == 1 and rms(D=254) == 1        # D % 4
    assert rms(dy=A + 4) == 1 and rms(x=B + 8) == 1 and rms(w=W + 4) == 1
    assert rms(wf=64 * 256 - 1, rstd=A) == 1                          # the slabs do not fit
    assert rms(wf=64 * 256) == 1                                      # ... nor, without rstd, the recomputed statistics behind them

    def col(x=A, ld=264, out=C, w=W, R=R, Cn=256):
        return lib.tasu_f32_colsum_split(x, ld, out, w, R, Cn, 0, None)

    assert col(x=None) == 1 and col(out=None) == 1 and col(w=None) == 1
    assert col(R=0) == 1 and col(Cn=0) == 1 and col(Cn=254) == 1 and col(ld=262) == 1 and col(ld=252) == 1
    assert col(x=A + 4) == 1 and col(w=W + 8) == 1
