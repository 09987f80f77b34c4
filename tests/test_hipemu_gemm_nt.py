"""CPU: the SOURCE of the large-minibatch trunk products (seqdex_amd/csrc/sdx_gemm_nt.h: k_gemm_nt, k_stage) executed on the SIMT
emulator (tests/hipemu: MFMA as a wave collective with the ISA's lane layouts, global_load_lds as the lane-linear copy it is) against
numpy: source-side swizzle vs fragment reads, accumulator layout, the three epilogues incl. the transposed copies and the ones-MFMA
row sums, split reductions, ragged edges, both element types.  What the emulator cannot show - bank conflicts, timing - is measured on
the GPU (profiles/r4_bigmb_*).  The cases and what they assert live in tests/gemm_nt_cases.py: tests/test_gpu_gemm_products.py runs the
same ones on the COMPILED kernels (where the emulator build's replacements under #ifdef HIPEMU - the v_dot2c row sums, global_load_lds -
are the real instructions), and the GPU parity tests (tests/test_gpu_ppo_parity.py::test_large_minibatch_*,
tests/test_gpu_ppo_branches.py) hold the assembled step to the autograd oracle on every path."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gemm_nt_cases as GC  # noqa: E402
from gemm_nt_cases import elems as _elems, from_elems as _from_elems  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"), reason="needs ROCm's clang++ for the host build")


@pytest.fixture(scope="module")
def lib():
    from tests import hipemu
    l = C.CDLL(hipemu.build_gemm())
    vp, i, fp = C.c_void_p, C.c_int, C.c_void_p
    l.emu_gemm_nt.argtypes = [i, i, C.POINTER(GC.NtArgs), i, i, i]
    l.emu_gemm_tt.argtypes = [C.POINTER(GC.NtArgs), i, i, i]
    l.emu_stage.argtypes = [i, fp, i, i, i, i, vp, i, vp, i]
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Emulated:
    """backend of gemm_nt_cases: 1..3 products per launch, at any tile, through the header's launchers (tests/hipemu/gemm_driver.cpp)"""

    def __init__(self, lib):
        self.lib = lib

    @staticmethod
    def _args(problems):
        return (GC.NtArgs * len(problems))(*[GC.nt_args(g, lambda k: None if getattr(g, k) is None else getattr(g, k).ctypes.data) for g in problems])

    def nt(self, bf, epi, tile, splits, problems):
        self.lib.emu_gemm_nt(bf, epi, self._args(problems), len(problems), splits, tile)

    def tt(self, tile, splits, problems):
        self.lib.emu_gemm_tt(self._args(problems), len(problems), splits, tile)


@pytest.fixture(scope="module")
def emu(lib):
    return Emulated(lib)


@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("M,N,K", GC.FORWARD_SHAPES)
def test_forward_product_all_outputs(emu, bf, M, N, K):
    GC.forward_product_all_outputs(emu, bf, M, N, K)


@pytest.mark.parametrize("bf", GC.BF)
def test_narrow_tile_shape(emu, bf):
    GC.narrow_tile_shape(emu, bf)


@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("epi", GC.WIDE_EPIS)
@pytest.mark.parametrize("M", GC.WIDE_M)
def test_wide_tile_shape_all_copies(emu, bf, epi, M):
    GC.wide_tile_shape_all_copies(emu, bf, epi, M)


@pytest.mark.parametrize("bf", GC.BF)
def test_data_gradient_product(emu, bf):
    GC.data_gradient_product(emu, bf)


@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("splits", GC.SPLITS)
def test_weight_gradient_product_with_row_sums(emu, bf, splits):
    GC.weight_gradient_product_with_row_sums(emu, bf, splits)


@pytest.mark.parametrize("bf", [0, 1])
def test_stage_kernel(lib, bf):
    rng = np.random.default_rng(3)
    R, K, lds = 150, 100, 104
    KC = 64 if bf else 32
    Kp = (K + KC - 1) // KC * KC
    src = rng.standard_normal((R, lds)).astype(np.float32)
    ldt = 200
    dn = np.full((R, Kp), 77, np.int16 if bf else np.float32)
    dt = np.zeros((Kp, ldt), np.int16 if bf else np.float32)
    lib.emu_stage(bf, _p(src), lds, R, K, Kp, _p(dn), Kp, _p(dt), ldt)
    _, want = _elems(src[:, :K], bf)
    n, t = _from_elems(dn, bf), _from_elems(dt, bf)
    np.testing.assert_array_equal(n[:, :K], want)
    assert not n[:, K:].any()
    np.testing.assert_array_equal(t[:K, :R], want.T)
    assert not t[K:].any() and not t[:, R:].any()


@pytest.mark.parametrize("tile", [1, 2, 0])
@pytest.mark.parametrize("R,Nl,Kl,ldb,splits", GC.TT_SHAPES)
def test_weight_gradient_from_row_major_operands(emu, tile, R, Nl, Kl, ldb, splits):
    GC.weight_gradient_from_row_major_operands(emu, tile, R, Nl, Kl, ldb, splits)


# ---- the cases above at the tiles they do not name, and the ones with three products per launch: what tests/test_gpu_gemm_products.py
# runs on the compiled kernels (tile 1 = 128 x 64, 2 = 128 x 128)
TILES = [1, 2]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("M,N,K", GC.FORWARD_SHAPES)
def test_forward_product_all_outputs_at_tile(emu, bf, M, N, K, tile):
    GC.forward_product_all_outputs(emu, bf, M, N, K, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
def test_forward_products_of_three_shapes_in_one_launch(emu, bf, tile):
    GC.forward_products_of_three_shapes_in_one_launch(emu, bf, tile)


@pytest.mark.parametrize("bf", GC.BF)
def test_narrow_tile_shape_at_wide_tile(emu, bf):
    GC.narrow_tile_shape(emu, bf, 2)


@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("epi", GC.WIDE_EPIS)
@pytest.mark.parametrize("M", GC.WIDE_M)
def test_wide_tile_shape_all_copies_at_narrow_tile(emu, bf, epi, M):
    GC.wide_tile_shape_all_copies(emu, bf, epi, M, 1)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("epi", GC.WIDE_EPIS)
@pytest.mark.parametrize("M", GC.WIDE_M)
def test_wide_tile_shape_odd_leading_dimensions(emu, bf, epi, M, tile):
    GC.wide_tile_shape_odd_leading_dimensions(emu, bf, epi, M, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
def test_data_gradient_product_at_tile(emu, bf, tile):
    GC.data_gradient_product(emu, bf, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("splits", GC.SPLITS)
def test_weight_gradient_product_with_row_sums_at_tile(emu, bf, splits, tile):
    GC.weight_gradient_product_with_row_sums(emu, bf, splits, tile)


@pytest.mark.parametrize("tile", TILES)
def test_weight_gradients_of_three_shapes_in_one_launch(emu, tile):
    GC.weight_gradients_of_three_shapes_in_one_launch(emu, tile)
