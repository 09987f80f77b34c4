"""Shared cases of the large-minibatch trunk products (seqdex_amd/csrc/sdx_gemm_nt.h: k_gemm_nt, k_gemm_tt): shapes, epilogues, splits,
tiles and element types, with what every case asserts.  tests/test_hipemu_gemm_nt.py runs them on the SIMT emulator (the SOURCE),
tests/test_gpu_gemm_products.py through sdxpk_gemm_nt_launch / sdxpk_gemm_tt_launch (the COMPILED kernels).  A `backend` has

    nt(bf, epi, tile, splits, problems)      k_gemm_nt on a list of 1..3 Problem (one launch)
    tt(tile, splits, problems)               k_gemm_tt likewise

and leaves the results in the numpy arrays of the problems.  tile: 0 = the launcher's choice, 1 = 128 x 64, 2 = 128 x 128.  The reference
is numpy in float64; for bf16 the operands ARE bf16 values, so products are exact and only the fp32 accumulation rounds."""
import ctypes as C

import numpy as np
import torch

EPI_FWD, EPI_NN, EPI_TN = 1, 3, 4


class NtArgs(C.Structure):      # sdx_gemm_nt.h
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int), ("B", C.c_void_p), ("ldb", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("kchunk", C.c_int), ("Cf", C.c_void_p), ("ldc", C.c_int), ("cz", C.c_size_t), ("Cn", C.c_void_p), ("ldn", C.c_int),
                ("Ct", C.c_void_p), ("ldt", C.c_int), ("bias", C.c_void_p), ("H", C.c_void_p), ("ldh", C.c_int), ("Ht", C.c_void_p), ("ldht", C.c_int),
                ("rowsum", C.c_void_p)]


def nt_args(g, address):
    """the NtArgs of Problem g; address(name): where the backend keeps the array g.<name> (None for a null pointer)"""
    return NtArgs(address("A"), g.lda, address("B"), g.ldb, g.M, g.N, g.K, g.kchunk, address("Cf"), g.ldc, g.cz, address("Cn"), g.ldn, address("Ct"), g.ldt,
                  address("bias"), address("H"), g.ldh, address("Ht"), g.ldht, None if g.rowsum_off is None else address("Cf") + 4 * g.rowsum_off)

BF = [0, 1]
FORWARD_SHAPES = [(128, 128, 128), (200, 150, 192), (70, 36, 64)]
WIDE_EPIS = [EPI_FWD, EPI_NN]
WIDE_M = [270, 272]
SPLITS = [1, 3]
TT_SHAPES = [(200, 128, 100, 128, 2), (96, 256, 396, 416, 1), (328, 128, 130, 160, 3)]      # R, Nl, Kl, ldb, splits


class Problem:
    """one product of a launch: the fields of NtArgs as numpy arrays (None: null pointer).  rowsum_off: the row sums go to Cf's buffer at
    this float offset (the [G | b] layout of a split partial)"""

    def __init__(self, A, lda, B, ldb, M, N, K, kchunk, Cf=None, ldc=0, cz=0, Cn=None, ldn=0, Ct=None, ldt=0, bias=None, H=None, ldh=0, Ht=None,
                 ldht=0, rowsum_off=None):
        self.__dict__.update(locals())
        del self.__dict__["self"]


def elems(x, bf):
    """(array handed to the kernel, float64 values it represents)"""
    t = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32)
    if bf:
        b = t.to(torch.bfloat16)
        return b.view(torch.int16).numpy().copy(), b.to(torch.float64).numpy()
    return t.numpy().copy(), t.to(torch.float64).numpy()


def from_elems(arr, bf):
    if bf:
        return torch.as_tensor(arr).view(torch.bfloat16).to(torch.float64).numpy()
    return arr.astype(np.float64)


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def forward_problem(rng, bf, M, N, K):
    """(Problem, check): a forward product with all three outputs; check() after the launch"""
    KC = 64 if bf else 32
    assert K % KC == 0
    A, Av = elems(rng.standard_normal((M, K)) * 0.5, bf)
    B, Bv = elems(rng.standard_normal((N, K)) * 0.5, bf)
    bias = rng.standard_normal(N).astype(np.float32)
    Mp = (M + 63) // 64 * 64
    Cf = np.full((M, N), np.nan, np.float32)
    Cn = np.zeros((M, N), np.int16 if bf else np.float32)
    Ct = np.zeros((N, Mp), np.int16 if bf else np.float32)

    def check():
        want = elu(Av @ Bv.T + bias)
        np.testing.assert_allclose(Cf, want, rtol=1e-5, atol=2e-5)      # (bf16: the operands ARE bf16 values, products exact, fp32 accumulation)
        got_n, got_t = from_elems(Cn, bf), from_elems(Ct, bf)
        np.testing.assert_allclose(got_n, Cf.astype(np.float64), rtol=8e-3 if bf else 0, atol=0)          # the copies are the fp32 result, rounded
        np.testing.assert_allclose(got_t[:, :M], Cf.astype(np.float64).T, rtol=8e-3 if bf else 0, atol=0)
        assert not got_t[:, M:].any()                                                                     # padding columns are never written
    return Problem(A, K, B, K, M, N, K, K, Cf, N, 0, Cn, N, Ct, Mp, bias), check


def forward_product_all_outputs(backend, bf, M, N, K, tile=0):
    g, check = forward_problem(np.random.default_rng(M + N + bf), bf, M, N, K)
    backend.nt(bf, EPI_FWD, tile, 1, [g])
    check()


def forward_products_of_three_shapes_in_one_launch(backend, bf, tile):
    """count = 3: the grid covers the largest M and the largest N of the batch, which here belong to different products; every workgroup
    past a product's own edge leaves"""
    rng = np.random.default_rng(29 + bf)
    three = [forward_problem(rng, bf, M, N, K) for M, N, K in ((200, 150, 192), (70, 36, 64), (130, 260, 128))]
    backend.nt(bf, EPI_FWD, tile, 1, [g for g, _ in three])
    for _, check in three:
        check()


def narrow_tile_shape(backend, bf, tile=1):
    rng = np.random.default_rng(5)
    M, N, K = 140, 100, 128
    A, Av = elems(rng.standard_normal((M, K)), bf)
    B, Bv = elems(rng.standard_normal((N, K)), bf)
    bias = np.zeros(N, np.float32)
    Cf = np.zeros((M, N), np.float32)
    Ct = np.zeros((N, 192), np.int16 if bf else np.float32)
    backend.nt(bf, EPI_FWD, tile, 1, [Problem(A, K, B, K, M, N, K, K, Cf, N, 0, None, 0, Ct, 192, bias)])
    np.testing.assert_allclose(Cf, elu(Av @ Bv.T), rtol=1e-5, atol=5e-5)
    np.testing.assert_allclose(from_elems(Ct, bf)[:, :M], Cf.astype(np.float64).T, rtol=8e-3 if bf else 0)


def wide_tile_shape_all_copies(backend, bf, epi, M, tile=2, odd=False):
    """the 128 x 128 tile: two passes of the transposed epilogue (64 columns each), 19 workgroups through the XCD remap, ragged edges
    (M = 270) and whole 16-byte pieces along the rows (M = 272).  odd: every leading dimension of the epilogue is odd in 16-byte pieces
    (ldc = ldn = ldh = N + 1, ldt = ldht = Mp + 2), so that every piece of H / Ht is loaded and every piece of Cf / Cn / Ct stored
    element by element; else they are whole pieces and the copy's row stride differs from the fp32 result's"""
    rng = np.random.default_rng(17 + bf + epi)
    N, K = 300, 128
    A, Av = elems(rng.standard_normal((M, K)) * 0.4, bf)
    B, Bv = elems(rng.standard_normal((N, K)) * 0.4, bf)
    bias = rng.standard_normal(N).astype(np.float32)
    Hd, Hv = elems(rng.standard_normal((M, N)), bf)
    ldc, ldn, ldh, Mp = (N + 1, N + 1, N + 1, 322) if odd else (N, N + 4, N, 320)
    H = np.zeros((M, ldh), Hd.dtype); H[:, :N] = Hd
    Ht = np.zeros((N, Mp), Hd.dtype); Ht[:, :M] = Hd.T                       # the layer output's transposed copy, as the forward product leaves it
    Cf = np.full((M, ldc), np.nan, np.float32)
    Cn = np.zeros((M, ldn), np.int16 if bf else np.float32)
    Ct = np.zeros((N, Mp), np.int16 if bf else np.float32)
    backend.nt(bf, epi, tile, 1, [Problem(A, K, B, K, M, N, K, K, Cf if epi == EPI_FWD else None, ldc, 0, Cn, ldn, Ct, Mp, bias, H, ldh, Ht, Mp)])
    want = elu(Av @ Bv.T + bias) if epi == EPI_FWD else (Av @ Bv.T) * np.where(Hv > 0, 1.0, Hv + 1.0)
    if epi == EPI_FWD:
        np.testing.assert_allclose(Cf[:, :N], want, rtol=1e-5, atol=2e-5)
    else:
        assert np.isnan(Cf).all()                                            # a product without an fp32 result writes none
    if odd:
        assert np.isnan(Cf[:, N:]).all()                                     # the padding column of every row stays as it was
    np.testing.assert_allclose(from_elems(Cn, bf)[:, :N], want, rtol=8e-3 if bf else 1e-5, atol=1e-3 if bf else 2e-5)
    assert not from_elems(Cn, bf)[:, N:].any()
    np.testing.assert_array_equal(from_elems(Ct, bf)[:, :M], from_elems(Cn, bf)[:, :N].T)
    assert not from_elems(Ct, bf)[:, M:].any()


def wide_tile_shape_odd_leading_dimensions(backend, bf, epi, M, tile=2):
    """wide_tile_shape_all_copies where no row of H, Ht, Cf, Cn or Ct but the first begins on a 16-byte piece: the scalar fallbacks of
    the epilogue's piece loads and stores, whole and ragged, in both orientations"""
    wide_tile_shape_all_copies(backend, bf, epi, M, tile, odd=True)


def data_gradient_product(backend, bf, tile=0):
    """dX = (dY W) * ELU'(H): A = dY [M][Nl], B = W^T [Kl][Nl]; outputs: element copy + transposed copy, no fp32 array"""
    rng = np.random.default_rng(7)
    M, Nl, Kl = 160, 128, 200
    A, Av = elems(rng.standard_normal((M, Nl)) * 0.3, bf)
    B, Bv = elems(rng.standard_normal((Kl, Nl)) * 0.3, bf)
    H, Hv = elems(rng.standard_normal((M, Kl)), bf)         # the layer output in the element type of the run
    Mp = 192
    Ht = np.zeros((Kl, Mp), H.dtype); Ht[:, :M] = H.T
    Cn = np.zeros((M, Kl), np.int16 if bf else np.float32)
    Ct = np.zeros((Kl, Mp), np.int16 if bf else np.float32)
    backend.nt(bf, EPI_NN, tile, 1, [Problem(A, Nl, B, Nl, M, Kl, Nl, Nl, None, 0, 0, Cn, Kl, Ct, Mp, None, H, Kl, Ht, Mp)])
    want = (Av @ Bv.T) * np.where(Hv > 0, 1.0, Hv + 1.0)
    np.testing.assert_allclose(from_elems(Cn, bf), want, rtol=8e-3 if bf else 1e-5, atol=1e-3 if bf else 2e-5)
    np.testing.assert_array_equal(from_elems(Ct, bf)[:, :M], from_elems(Cn, bf).T)
    assert not from_elems(Ct, bf)[:, M:].any()


def weight_gradient_product_with_row_sums(backend, bf, splits, tile=0):
    """G = dY^T X over the minibatch rows: A = dY^T [Nl][MBp], B = X^T [Kl][ld], split over the rows; the row sums of A (bias gradient)
    come from the first column block, beside the MFMAs"""
    rng = np.random.default_rng(11 + splits)
    KC = 64 if bf else 32
    Nl, Kl, MB = 128, 140, 3 * KC - 8                      # ragged minibatch: the last chunk is zero padded in A
    MBp = (MB + KC - 1) // KC * KC
    A0 = np.zeros((Nl, MBp)); A0[:, :MB] = rng.standard_normal((Nl, MB)) * 0.5
    ldb = MBp + 64
    B0 = rng.standard_normal((Kl, ldb))                     # what follows the window in a transposed dataset: finite, multiplied by A's zeros
    A, Av = elems(A0, bf)
    B, Bv = elems(B0, bf)
    kc = ((MBp + splits - 1) // splits + KC - 1) // KC * KC
    pz = Nl * Kl + Nl
    part = np.full((splits, pz), np.nan, np.float32)
    backend.nt(bf, EPI_TN, tile, splits, [Problem(A, MBp, B, ldb, Nl, Kl, MBp, kc, part, Kl, pz, rowsum_off=Nl * Kl)])
    assert np.isfinite(part).all()
    tot = part.astype(np.float64).sum(0)
    G, rs = tot[:Nl * Kl].reshape(Nl, Kl), tot[Nl * Kl:]
    np.testing.assert_allclose(G, Av @ Bv[:, :MBp].T, rtol=1e-5, atol=5e-5)
    np.testing.assert_allclose(rs, Av.sum(1), rtol=1e-5, atol=1e-4)


def tt_problem(rng, R, Nl, Kl, ldb, splits):
    """(Problem, check) of k_gemm_tt: G [Nl][Kl] = dY^T X over R rows in `splits` row ranges, partials [G | b] per split"""
    A = (rng.standard_normal((R, Nl)) * 0.3).astype(np.float32)
    B = np.full((R, ldb), np.nan, np.float32)                       # padding columns hold garbage in the real buffers of layers > 0 ...
    B[:, :Kl] = rng.standard_normal((R, Kl)).astype(np.float32)
    B[:, Kl:] = 7.0                                                 # ... here a finite marker: products with it belong to outputs that are never stored
    kchunk = ((R + splits - 1) // splits + 31) // 32 * 32
    pz = Nl * Kl + Nl
    part = np.full((splits, pz), np.nan, np.float32)

    def check():
        assert np.isfinite(part).all()
        tot = part.sum(0)
        want = A.astype(np.float64).T @ B[:, :Kl].astype(np.float64)
        np.testing.assert_allclose(tot[:Nl * Kl].reshape(Nl, Kl), want, rtol=1e-5, atol=3e-5)
        np.testing.assert_allclose(tot[Nl * Kl:], A.astype(np.float64).sum(0), rtol=1e-5, atol=3e-5)
        for z in range(splits):                                         # every split covers exactly its own rows
            r0, r1 = z * kchunk, min(R, (z + 1) * kchunk)
            np.testing.assert_allclose(part[z, :Nl * Kl].reshape(Nl, Kl), A[r0:r1].astype(np.float64).T @ B[r0:r1, :Kl].astype(np.float64), rtol=1e-5, atol=3e-5)
    return Problem(A, Nl, B, ldb, Nl, Kl, R, kchunk, part, Kl, pz, rowsum_off=Nl * Kl), check


def weight_gradient_from_row_major_operands(backend, tile, R, Nl, Kl, ldb, splits):
    """k_gemm_tt (fp32): G = dY^T X read from dY [rows][N_l] and X [rows][K_l] as the other products leave them - no transposed copies.
    Ragged rows (the last chunk comes partly from the page of zeros), columns past the operand's width clamped into it, row splits,
    both tiles, column sums of dY (the bias gradient) beside the MFMAs."""
    g, check = tt_problem(np.random.default_rng(R + Kl + tile), R, Nl, Kl, ldb, splits)
    backend.tt(tile, splits, [g])
    check()


def weight_gradients_of_three_shapes_in_one_launch(backend, tile):
    """count = 3 on k_gemm_tt, two row ranges each: the widest G and the tallest G belong to different products"""
    rng = np.random.default_rng(31)
    three = [tt_problem(rng, R, Nl, Kl, ldb, 2) for R, Nl, Kl, ldb in ((200, 128, 100, 128), (72, 256, 40, 64), (136, 128, 396, 416))]
    backend.tt(tile, 2, [g for g, _ in three])
    for _, check in three:
        check()
