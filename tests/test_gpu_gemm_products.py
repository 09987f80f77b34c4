"""-m gpu: every product kernel of the large-minibatch PPO step and of the T-value trainer, COMPILED, one launch at a time against float64.

k_gemm_nt / k_gemm_tt (sdx_gemm_nt.h): the cases of tests/gemm_nt_cases.py - the ones tests/test_hipemu_gemm_nt.py runs on the emulator,
with the same bounds - through sdxpk_gemm_nt_launch / sdxpk_gemm_tt_launch, each at both tiles, plus three products of different shapes
in one launch.  Here the row sums are v_dot2c_f32_bf16, the loads global_load_lds and the 1-D grid goes through the dispatcher, which
the emulator build replaces.

k_gemm (sdx_gemm.h), which no emulator test covers: every instantiated (AT, BT, EPI) product at tile 64 x 64, 128 x 64 and 128 x 128, fp32
and bf16 (BF = 1 rounds on the load path), through sdxpk_gemm_launch at the shapes the step and the trainer give it and their ragged
neighbours.  Inputs carry NaN in their padding, outputs are pre-filled with NaN: nothing outside [M, N] may be written, nothing outside
the operands read.  The bound is derived per output, not tuned: a reduction of K fma steps in fp32 is within K 2^-24 (|A| |B|^T)[i][j] of
the exact product of the operands as the kernel sees them (for BF = 1: rounded to bf16 by torch, round to nearest even as v_cvt_pk_bf16_f32),
plus 4 ulp of the result where an epilogue adds a bias, an ELU or an ELU'.  A dropped reduction index costs about (|A| |B|^T) / K: far
outside.  Every case prints its largest error / bound ratio (profiles/gemm_products_gpu_bounds.txt)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gemm_nt_cases as GC  # noqa: E402


NtArgs = GC.NtArgs              # sdx_gemm_nt.h


class GemmArgs(C.Structure):    # sdx_gemm.h
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int), ("B", C.c_void_p), ("ldb", C.c_int), ("C", C.c_void_p), ("ldc", C.c_int), ("cz", C.c_size_t),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("kchunk", C.c_int), ("bias", C.c_void_p), ("H", C.c_void_p), ("ldh", C.c_int),
                ("rowsum", C.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    from seqdex_amd import _abi
    l = _abi.load_library()
    i, vp = C.c_int, C.c_void_p
    l.sdxpk_gemm_nt_launch.restype = l.sdxpk_gemm_tt_launch.restype = l.sdxpk_gemm_launch.restype = i
    l.sdxpk_gemm_nt_launch.argtypes = [i, i, C.POINTER(NtArgs), i, i, i, vp]
    l.sdxpk_gemm_tt_launch.argtypes = [C.POINTER(NtArgs), i, i, vp, i, vp]
    l.sdxpk_gemm_launch.argtypes = [i, i, i, i, C.POINTER(GemmArgs), i, i, i, vp]
    return l


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Compiled:
    """backend of gemm_nt_cases on the GPU: the numpy arrays of every problem go to the device, one launch, the outputs come back"""

    def __init__(self, lib):
        self.lib = lib
        self.zeros = torch.zeros(64, device="cuda")

    def _launch(self, problems, call):
        dev, outs = [], []
        arr = (NtArgs * 3)()
        for q, g in enumerate(problems):
            t = {k: torch.from_numpy(getattr(g, k)).cuda() for k in ("A", "B", "Cf", "Cn", "Ct", "bias", "H", "Ht") if getattr(g, k) is not None}
            arr[q] = GC.nt_args(g, lambda k: t[k].data_ptr() if k in t else None)
            dev.append(t)
            outs += [(getattr(g, k), t[k]) for k in ("Cf", "Cn", "Ct") if k in t]
        assert call(arr, len(problems)) == 0
        torch.cuda.synchronize()
        for host, t in outs:
            host[...] = t.cpu().numpy()

    def nt(self, bf, epi, tile, splits, problems):
        self._launch(problems, lambda arr, n: self.lib.sdxpk_gemm_nt_launch(bf, epi, arr, n, splits, tile, _stream()))

    def tt(self, tile, splits, problems):
        self._launch(problems, lambda arr, n: self.lib.sdxpk_gemm_tt_launch(arr, n, splits, self.zeros.data_ptr(), tile, _stream()))


@pytest.fixture(scope="module")
def gpu(lib):
    return Compiled(lib)


TILES = [1, 2]      # 128 x 64, 128 x 128


# ---------------------------------------------------------------------------------------------------- k_gemm_nt, k_gemm_tt
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("M,N,K", GC.FORWARD_SHAPES)
def test_forward_product_all_outputs(gpu, bf, M, N, K, tile):
    GC.forward_product_all_outputs(gpu, bf, M, N, K, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
def test_forward_products_of_three_shapes_in_one_launch(gpu, bf, tile):
    GC.forward_products_of_three_shapes_in_one_launch(gpu, bf, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
def test_narrow_tile_shape(gpu, bf, tile):
    GC.narrow_tile_shape(gpu, bf, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("epi", GC.WIDE_EPIS)
@pytest.mark.parametrize("M", GC.WIDE_M)
def test_wide_tile_shape_all_copies(gpu, bf, epi, M, tile):
    GC.wide_tile_shape_all_copies(gpu, bf, epi, M, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("epi", GC.WIDE_EPIS)
@pytest.mark.parametrize("M", GC.WIDE_M)
def test_wide_tile_shape_odd_leading_dimensions(gpu, bf, epi, M, tile):
    GC.wide_tile_shape_odd_leading_dimensions(gpu, bf, epi, M, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
def test_data_gradient_product(gpu, bf, tile):
    GC.data_gradient_product(gpu, bf, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("splits", GC.SPLITS)
def test_weight_gradient_product_with_row_sums(gpu, bf, splits, tile):
    GC.weight_gradient_product_with_row_sums(gpu, bf, splits, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("R,Nl,Kl,ldb,splits", GC.TT_SHAPES)
def test_weight_gradient_from_row_major_operands(gpu, tile, R, Nl, Kl, ldb, splits):
    GC.weight_gradient_from_row_major_operands(gpu, tile, R, Nl, Kl, ldb, splits)


@pytest.mark.parametrize("tile", TILES)
def test_weight_gradients_of_three_shapes_in_one_launch(gpu, tile):
    GC.weight_gradients_of_three_shapes_in_one_launch(gpu, tile)


def test_hooks_refuse_what_is_not_instantiated(lib):
    g = (GemmArgs * 3)()
    n = (NtArgs * 3)()
    assert lib.sdxpk_gemm_launch(1, 0, 1, 0, g, 1, 1, 0, None) == -1       # no (AT, BT, EPI) = (1, 0, 1) product exists
    assert lib.sdxpk_gemm_launch(0, 0, 1, 0, g, 1, 1, 4, None) == -1       # tiles are 0 .. 3
    assert lib.sdxpk_gemm_launch(0, 0, 1, 0, g, 4, 1, 0, None) == -1       # a launch holds up to three products
    assert lib.sdxpk_gemm_tt_launch(n, 1, 1, None, 1, None) == -1          # k_gemm_tt needs its page of zeros
    assert lib.sdxpk_gemm_nt_launch(0, 2, n, 1, 1, 1, None) == -1


# ---------------------------------------------------------------------------------------------------- k_gemm
U24 = 2.0 ** -24
K_TILES = [1, 2, 3]     # 64 x 64, 128 x 64, 128 x 128
FWD, BIAS, DGRAD, WGRAD = (0, 0, 1), (0, 0, 2), (0, 1, 3), (1, 1, 4)


def _store(x, transposed, ld, offset=0):
    """logical x [rows][k] -> the kernel's array ([rows][ld], or [k][ld] when transposed), NaN in the padding; `offset` floats into its buffer"""
    x = x.t() if transposed else x
    buf = torch.full((offset + x.shape[0] * ld,), float("nan"))
    buf[offset:].view(x.shape[0], ld)[:, :x.shape[1]] = x
    return buf


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, seed):
    """A [M][K], B [N][K], bias [N], H [M][N] (a layer output: both signs) - drawn once per shape, never written"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, K, generator=g) * 0.5, torch.randn(N, K, generator=g) * 0.5, torch.randn(N, generator=g),
            torch.randn(M, N, generator=g))


def run_k_gemm(lib, product, bf, tile, M, N, K, lda=None, ldb=None, ldc=None, splits=1, a_offset=0):
    at, bt, epi = product
    A, B, bias, H = _operands(M, N, K, 1000 * M + N + K)
    lda, ldb, ldc = lda or (M if at else K), ldb or (N if bt else K), ldc or N
    kchunk = (K + splits - 1) // splits
    cz = M * ldc + M if epi == 4 else 0                       # a split partial: [G | row sums]
    A_d, B_d = _store(A, at, lda, a_offset).cuda(), _store(B, bt, ldb).cuda()
    bias_d, H_d = bias.cuda(), H.contiguous().cuda()
    out = torch.full((splits, max(cz, M * ldc)), float("nan"), device="cuda")
    a = GemmArgs(A_d.data_ptr() + 4 * a_offset, lda, B_d.data_ptr(), ldb, out.data_ptr(), ldc, cz, M, N, K, kchunk,
                 bias_d.data_ptr() if epi in (1, 2) else None, H_d.data_ptr() if epi == 3 else None, N, out.data_ptr() + 4 * M * ldc if epi == 4 else None)
    assert lib.sdxpk_gemm_launch(at, bt, epi, bf, (GemmArgs * 3)(a, a, a), 1, splits, tile, _stream()) == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy().astype(np.float64)
    rnd = (lambda x: x.to(torch.bfloat16)) if bf else (lambda x: x)
    Av, Bv = rnd(A).double().numpy(), rnd(B).double().numpy()
    worst = 0.0
    for z in range(splits):
        k0, k1 = z * kchunk, min(K, (z + 1) * kchunk)
        acc, mag = Av[:, k0:k1] @ Bv[:, k0:k1].T, np.abs(Av[:, k0:k1]) @ np.abs(Bv[:, k0:k1]).T
        if epi in (1, 2):
            acc = acc + bias.double().numpy()
        want = GC.elu(acc) if epi == 1 else acc * np.where(H.numpy() > 0, 1.0, H.double().numpy() + 1.0) if epi == 3 else acc
        bound = (k1 - k0) * U24 * mag + (4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) if epi in (1, 2, 3) else 0.0)
        got = out[z, :M * ldc].reshape(M, ldc)
        assert np.isnan(got[:, N:]).all(), "written outside [M, N]"
        err = np.abs(got[:, :N] - want)
        assert np.isfinite(err).all()
        worst = max(worst, float((err / bound).max()))
        if epi == 4:
            rs_err = np.abs(out[z, M * ldc:M * ldc + M] - Av[:, k0:k1].sum(1))
            worst = max(worst, float((rs_err / ((k1 - k0) * U24 * np.abs(Av[:, k0:k1]).sum(1))).max()))
            assert np.isnan(out[z, M * ldc + M:]).all()
        else:
            assert np.isnan(out[z, M * ldc:]).all()
    print("k_gemm ratio product %s bf %d tile %d M %d N %d K %d lda %d splits %d offset %d: largest error / bound %.3f"
          % (product, bf, tile, M, N, K, lda, splits, a_offset, worst))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("tile", K_TILES)
@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("N,K", [(128, 100), (256, 396)])
@pytest.mark.parametrize("M", [12, 72, 136])
@pytest.mark.parametrize("product", [FWD, DGRAD], ids=["forward", "data_gradient"])
def test_k_gemm_trunk_forward_and_data_gradient(lib, product, M, N, K, bf, tile):
    """the trunk on the k_gemm path (minibatches that are no multiple of 8, SDXP_BIGMB_NT=0): 12 rows in one tile, 72 = 64 + 8, 136 = 128 + 8;
    K = 100 ends inside a reduction chunk of every tile"""
    run_k_gemm(lib, product, bf, tile, M, N, K)


@pytest.mark.parametrize("tile", K_TILES)
@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("M", [12, 72, 136])
def test_k_gemm_mu_head(lib, M, bf, tile):
    """mu = h3 Wmu^T + b: 23 columns in rows of 24"""
    run_k_gemm(lib, BIAS, bf, tile, M, 23, 256, ldc=24)


@pytest.mark.parametrize("tile", K_TILES)
@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("M", [12, 72, 136])
def test_k_gemm_mu_head_data_gradient(lib, M, bf, tile):
    """dY2 = (dmu Wmu) * ELU'(h3): the reduction runs over 23 of the 24 floats of a dmu row - load4's scalar tail"""
    run_k_gemm(lib, DGRAD, bf, tile, M, 256, 23, lda=24)


@pytest.mark.parametrize("tile", K_TILES)
@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("M,N,lda", [(23, 256, 24), (128, 100, 128)])
def test_k_gemm_weight_gradient_with_row_sums(lib, M, N, lda, splits, bf, tile):
    """G = dY^T X over 136 rows, whole and in three ranges of 46 (no multiple of a reduction chunk), partials cz apart, the bias
    gradient as row sums; M = 23: the mu head's (dmu rows of 24 floats)"""
    run_k_gemm(lib, WGRAD, bf, tile, M, N, 136, lda=lda, splits=splits)


@pytest.mark.parametrize("tile", K_TILES)
@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("N,K", [(256, 4), (2, 64)])
@pytest.mark.parametrize("M", [2, 70])
def test_k_gemm_tvalue_layers(lib, M, N, K, bf, tile):
    """the T-value trainer's first and last layer: a reduction of 4, an output of 2 columns"""
    run_k_gemm(lib, FWD, bf, tile, M, N, K)


@pytest.mark.parametrize("tile", K_TILES)
@pytest.mark.parametrize("bf", [0, 1])
def test_k_gemm_operand_off_16_byte_alignment(lib, bf, tile):
    """A begins 4 bytes into its allocation: load4 takes its unaligned branch for every piece"""
    run_k_gemm(lib, FWD, bf, tile, 72, 128, 100, a_offset=1)
