"""-m gpu: the head matrix between the CUs of the persistent update kernel (csrc/sdxp_persist_exchange.h: head_owned, head_publish, head_rows_peek /
head_row24_peek / head_rows_take, head_cols_load).  Rows w, w + 8, w + 16 of one column of the 25 x 256 matrix travel in one tagged 16-byte word (word
256 w + c of the region LQ_HW), row 24 in 8-byte (value, tag) words; CU g owns the eight words 8 g .. 8 g + 7 - rows (g >> 5) + {0, 8, 16} of columns
8 (g & 31) .. + 7 - and column g of row 24.  Phase D takes the matrix twice: wave w its rows w + 8 j at columns lane + 64 e (wh[j][e], with the tags), lane
(column c2n, row half c2c) rows min(13 c2c + j, 24) (wc[j], plain dwords).

The test entries (csrc/sdxp_persist_checks.hip, built with the epoch kernel's flags) call those helpers in two launches in stream order, so no workgroup
waits for another inside a launch and nothing polls: (1) 256 workgroups publish a given matrix with a given tag through the ownership map, (2) one
workgroup of 512 threads takes the row view with the non-polling take and loads the column view.

The matrix holds 6 400 pairwise different bit patterns, among them -0.0, a denormal and a NaN with a payload, and everything is compared as bits: float
arithmetic on a value anywhere on the way (a flushed denormal, a quieted NaN, a lost sign of zero) fails the test.

(1) every wh[j][e] is W[wave + 8 j][lane + 64 e] (0 where the wave has no such row), every wc[j] is W[min(13 c2c + j, 24)][c2n], every wave's take hits;
(2) the ownership map, dumped as (row, column) per (CU, thread), covers each of the 6 400 elements exactly once;
(3) with CU 100's words published under tag - 1 the take misses on exactly waves 0 and 3 - CU 100 owns rows 3, 11, 19 (wave 3's) of columns 32..39 and
    column 100 of row 24 (wave 0's) - and hits on the others."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U2, ROWS, NTH, NWG, HPC, NWV = 256, 25, 512, 256, 25, 8
TAG = 0x01234567
STALE_CU = 100
STALE_WAVES = {STALE_CU >> 5, 0}   # the wave of its three rows, and wave 0 for its column of row 24


def _matrix():
    # 6 400 different patterns: ordinary floats of both signs with distinct mantissas, then the special ones
    r = np.random.default_rng(5)
    bits = (r.permutation(1 << 22)[:ROWS * U2].astype(np.uint32) | (r.integers(1, 250, ROWS * U2).astype(np.uint32) << 23)
            | (r.integers(0, 2, ROWS * U2).astype(np.uint32) << 31))
    bits[17] = 0x80000000        # -0.0
    bits[U2 * 11 + 200] = 0x00000001   # the smallest denormal
    bits[U2 * 24 + 100] = 0x7FA12345   # a signalling NaN with a payload
    bits[U2 * 19 + 33] = 0xFFC00BAD    # a quiet NaN with a payload, sign set
    bits[U2 * 24 + 7] = 0x807FFFFF     # the largest denormal, negative
    assert len(np.unique(bits)) == ROWS * U2
    return bits.reshape(ROWS, U2)


@pytest.fixture(scope="module")
def runs():
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib, dev = _abi.load_library(), torch.device("cuda:0")
    lib.sdxpk_head_words_ll_words.restype = C.c_size_t
    lib.sdxpk_head_publish_check.restype = C.c_int
    lib.sdxpk_head_publish_check.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sdxpk_head_views_check.restype = C.c_int
    lib.sdxpk_head_views_check.argtypes = [C.c_void_p, C.c_uint] + [C.c_void_p] * 4
    W = _matrix()
    Wd = torch.from_numpy(W.view(np.int32)).to(dev)
    st = _stream_ptr(dev)
    out = {}
    for name, stale in (("fresh", -1), ("stale", STALE_CU)):
        ll = torch.zeros(lib.sdxpk_head_words_ll_words(), dtype=torch.int64, device=dev)
        own = torch.full((NWG, HPC, 2), -1, dtype=torch.int32, device=dev)
        wh = torch.full((NTH, 4, 4), -1, dtype=torch.int32, device=dev)
        wc = torch.full((NTH, 13), -1, dtype=torch.int32, device=dev)
        verdict = torch.full((NWV,), -1, dtype=torch.int32, device=dev)
        assert lib.sdxpk_head_publish_check(Wd.data_ptr(), TAG, stale, ll.data_ptr(), own.data_ptr(), st) == 0
        assert lib.sdxpk_head_views_check(ll.data_ptr(), TAG, wh.data_ptr(), wc.data_ptr(), verdict.data_ptr(), st) == 0
        torch.cuda.synchronize()
        out[name] = tuple(v.cpu().numpy() for v in (own, wh, wc, verdict))
    return W, out


def _expected_views(W):
    t = np.arange(NTH)
    wave, lane = t >> 6, t & 63
    wh = np.zeros((NTH, 4, 4), np.uint32)
    for j in range(4):
        for e in range(4):
            row = wave + 8 * j
            ok = row < ROWS
            wh[ok, j, e] = W[row[ok], lane[ok] + 64 * e]
    c2c, c2n = (t >> 5) & 1, 32 * (t >> 6) + (t & 31)
    wc = np.stack([W[np.minimum(13 * c2c + j, ROWS - 1), c2n] for j in range(13)], axis=1)
    return wh, wc


def test_both_views_hold_the_published_elements(runs):
    W, out = runs
    _, wh, wc, verdict = out["fresh"]
    ewh, ewc = _expected_views(W)
    print("row view: %d of %d slots differ; column view: %d of %d" % (int((wh.view(np.uint32) != ewh).sum()), ewh.size, int((wc.view(np.uint32) != ewc).sum()), ewc.size))
    np.testing.assert_array_equal(wh.view(np.uint32), ewh)
    np.testing.assert_array_equal(wc.view(np.uint32), ewc)
    np.testing.assert_array_equal(verdict, np.ones(NWV, np.int32))


def test_ownership_covers_every_element_once(runs):
    _, out = runs
    own = out["fresh"][0].reshape(-1, 2).astype(np.int64)
    assert (own[:, 0] >= 0).all() and (own[:, 0] < ROWS).all() and (own[:, 1] >= 0).all() and (own[:, 1] < U2).all()
    count = np.bincount(own[:, 0] * U2 + own[:, 1], minlength=ROWS * U2)
    assert count.size == ROWS * U2 and (count == 1).all()
    # what the layout states: CU g holds rows (g >> 5) + {0, 8, 16} of columns 8 (g & 31) .. + 7, and column g of row 24
    g = np.arange(NWG)[:, None]
    t = np.arange(HPC - 1)[None, :]
    own = out["fresh"][0]
    np.testing.assert_array_equal(own[:, :HPC - 1, 0], (g >> 5) + 8 * (t >> 3))
    np.testing.assert_array_equal(own[:, :HPC - 1, 1], 8 * (g & 31) + (t & 7))
    np.testing.assert_array_equal(own[:, HPC - 1, 0], np.full(NWG, ROWS - 1))
    np.testing.assert_array_equal(own[:, HPC - 1, 1], np.arange(NWG))


def test_a_stale_producer_is_a_miss_on_its_readers_only(runs):
    W, out = runs
    _, wh, wc, verdict = out["stale"]
    print("verdict per wave with CU %d one tag behind: %s" % (STALE_CU, verdict.tolist()))
    np.testing.assert_array_equal(verdict, np.array([0 if w in STALE_WAVES else 1 for w in range(NWV)], np.int32))
    # the values travelled all the same: the tag is the only difference
    ewh, ewc = _expected_views(W)
    np.testing.assert_array_equal(wh.view(np.uint32), ewh)
    np.testing.assert_array_equal(wc.view(np.uint32), ewc)
