"""tiled, assert_tiles and the tiled CSR builders of gpu_support (no GPU): the layout the chip-filling and past-2^32
tests of tests/test_gpu_ct_scale.py are built on, and the proof that their comparator cannot pass a wrong slab, on torch
CPU tensors through an env whose device is the CPU."""
import numpy as np
import pytest
import torch

from gpu_support import SENTINEL, assert_tiles, slab_position, tiled, tiled_entries, tiled_idx, tiled_row_ptr

ENV = dict(torch=torch, dev=torch.device("cpu"))
K, ROWS, N, B = 3, 2, 8, 12


def base_records():
    """K distinct records [K][ROWS][N] of 32-bit words, the high bit set in some."""
    return np.random.default_rng(7).integers(0, 2 ** 32, (K, ROWS, N), dtype=np.uint64).astype(np.uint32)


def guarded_slab(base):
    """An exact tiling written into the head of a SENTINEL-filled buffer -> the [B][ROWS][N] view, the guard view."""
    buf = torch.full((B * ROWS * N + 2 * N,), SENTINEL, dtype=torch.int32)
    got = tiled(ENV, base, B, out=buf[:B * ROWS * N].view(B, ROWS, N))
    return got, buf[B * ROWS * N:]


def test_tiled_gives_record_b_equal_to_base_b_mod_k():
    base = base_records()
    got = tiled(ENV, base, B)
    assert tuple(got.shape) == (B, ROWS, N) and got.dtype == torch.int32 and got.is_contiguous()
    h = got.numpy().view(np.uint32)
    for b in range(B):
        assert (h[b] == base[b % K]).all(), b
    got, guard = guarded_slab(base)                                      # out=: the caller's buffer, nothing behind it
    assert (got.numpy().view(np.uint32) == np.tile(base, (B // K, 1, 1))).all() and bool((guard == SENTINEL).all())
    with pytest.raises(AssertionError):
        tiled(ENV, base, B + 1)                                          # B must be a multiple of K
    with pytest.raises(AssertionError):
        tiled(ENV, base, B, out=torch.empty((B, ROWS, N + 1), dtype=torch.int32))


@pytest.mark.parametrize("chunk_bytes", [1 << 30, 1], ids=["one-chunk", "a-tile-per-chunk"])
def test_assert_tiles_passes_an_exact_tiling(chunk_bytes):
    base = base_records()
    got, guard = guarded_slab(base)
    assert_tiles(ENV, got, base, "exact", guard=guard, chunk_bytes=chunk_bytes)
    assert_tiles(ENV, got, torch.from_numpy(base.view(np.int32)), "exact, tensor expectation", chunk_bytes=chunk_bytes)
    status = np.array([1, 0, 2], dtype=np.uint8)
    assert_tiles(ENV, tiled(ENV, status, B), status, "status bytes", chunk_bytes=chunk_bytes)
    f64 = np.array([[0.0, np.nan], [1.5, -2.0], [-0.0, 3.0]])
    assert_tiles(ENV, tiled(ENV, f64, B), f64, "doubles, by bit pattern", chunk_bytes=chunk_bytes)


@pytest.mark.parametrize("chunk_bytes", [1 << 30, 1], ids=["one-chunk", "a-tile-per-chunk"])
@pytest.mark.parametrize("record,row,word", [(B - 1, ROWS - 1, N - 1), (0, 0, 0), (B - 1, 0, 3)],
                         ids=["last-word-of-last-record", "first-word-of-first-record", "inside-last-record"])
def test_assert_tiles_names_one_changed_word(chunk_bytes, record, row, word):
    base = base_records()
    got, guard = guarded_slab(base)
    got[record, row, word] ^= 1
    with pytest.raises(AssertionError) as err:
        assert_tiles(ENV, got, base, "one word", guard=guard, chunk_bytes=chunk_bytes)
    text = str(err.value)
    assert f"1 of {B} records differ" in text and f"first bad record {record} " in text, text
    assert f"row {row}, word {word}:" in text and "(1 words of that record differ)" in text, text
    assert f"starts at word {record * ROWS * N} = byte {record * ROWS * N * 4} of the slab" in text, text
    assert "before byte 2^32, before word 2^31, before word 2^32" in text, text


def test_assert_tiles_fails_on_a_changed_guard_word():
    base = base_records()
    got, guard = guarded_slab(base)
    guard[-1] = 0
    assert_tiles(ENV, got, base, "no guard given")
    with pytest.raises(AssertionError, match="1 of the 16 guard words behind the result are written"):
        assert_tiles(ENV, got, base, "guard", guard=guard)


def test_assert_tiles_fails_on_two_swapped_records_of_one_tile():
    base = base_records()
    got, guard = guarded_slab(base)
    got[[7, 8]] = got[[8, 7]]                                            # tile 2: its records 1 and 2
    with pytest.raises(AssertionError) as err:
        assert_tiles(ENV, got, base, "swap", guard=guard)
    text = str(err.value)
    assert f"2 of {B} records differ" in text and "first bad record 7 (tile 2, pattern record 1)" in text, text


def test_assert_tiles_fails_on_a_float_that_differs_in_sign_of_zero_only():
    f32 = np.array([[0.0, 1.0], [2.0, 3.0]], dtype=np.float32)
    got = tiled(ENV, f32, 6)
    got[5, 0] = -0.0
    with pytest.raises(AssertionError, match="first bad record 5 "):
        assert_tiles(ENV, got, f32, "minus zero")


def test_position_report_names_the_three_thresholds():
    """slab_position, the sentence assert_tiles ends its report with, on records of 12 288 four-byte words (4096 x 3):
    record 87 381 is the last that starts before byte 2^32, 174 762 before word 2^31, 349 525 before word 2^32."""
    words = 3 * 4096
    for record, want in ((0, "before byte 2^32, before word 2^31, before word 2^32"),
                         (87381, "before byte 2^32, before word 2^31, before word 2^32"),
                         (87382, "at or past byte 2^32, before word 2^31, before word 2^32"),
                         (174762, "at or past byte 2^32, before word 2^31, before word 2^32"),
                         (174763, "at or past byte 2^32, at or past word 2^31, before word 2^32"),
                         (349525, "at or past byte 2^32, at or past word 2^31, before word 2^32"),
                         (349526, "at or past byte 2^32, at or past word 2^31, at or past word 2^32")):
        text = slab_position(record, words, 4)
        assert text == f"starts at word {record * words} = byte {record * words * 4} of the slab: {want}", record


def test_tiled_csr_rows_stay_inside_their_tile():
    local_ptr, local_idx, tiles = [0, 1, 3, 6], [2, 0, 1, 1, 1, 0], 4        # rows of 1, 2 and 3 records of a tile of K
    rp = tiled_row_ptr(ENV, local_ptr, tiles).numpy()
    ix = tiled_idx(ENV, local_idx, K, tiles).numpy()
    assert rp.dtype == np.int32 and ix.dtype == np.int32 and rp.shape == (tiles * 3 + 1,) and ix.shape == (tiles * 6,)
    for g in range(tiles * 3):
        t, r = divmod(g, 3)
        members = ix[rp[g]:rp[g + 1]]
        assert list(members - t * K) == local_idx[local_ptr[r]:local_ptr[r + 1]], g
        assert ((t * K <= members) & (members < (t + 1) * K)).all(), g
    assert rp[-1] == ix.size
    w = np.array([-2 ** 31, 2 ** 31 - 1, 0, 1, -1, 7], dtype=np.int32)
    assert (tiled_entries(ENV, w, tiles).numpy() == np.tile(w, tiles)).all()
    with pytest.raises(AssertionError):
        tiled_idx(ENV, [0, K], K, tiles)                                 # a local index outside the tile
