"""CPU: the restatement of the SEGCONV inference dropout (dropout_ref.py) against Random123's known answers and the
contract's properties, and ojf_segconv_set_dropout's argument check, which refuses a bad call before any HIP call."""
import numpy as np
import pytest

from online_joint_depthfusion_and_semantic_amd import _lib
from dropout_ref import counters, keep_mask, philox4x32_10

F32 = 0xffffffff


@pytest.mark.parametrize('ctr,key,want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((F32, F32, F32, F32), (F32, F32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    got = philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want


def test_philox_vectorises_like_scalar_calls():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 2 ** 32, size=(6, 4), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, size=(6, 2), dtype=np.uint64)
    batch = np.stack(philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), axis=1)
    for i in range(6):
        assert tuple(batch[i]) == tuple(philox4x32_10(*[int(v) for v in c[i]], *[int(v) for v in k[i]]))


@pytest.mark.parametrize('c_out', [1, 2, 3, 5, 6, 30, 512])
def test_counters_are_unique_per_pixel_and_group(c_out):
    n_pix = 257
    ctr = counters(n_pix, c_out)
    assert ctr.shape == (n_pix, (c_out + 3) // 4)
    assert np.unique(ctr).size == ctr.size
    assert int(ctr[0, 0]) == 0 and int(ctr[-1, -1]) == ctr.size - 1  # dense: pixel-major, then group


def test_element_numbering_is_word_c_mod_4_of_group_c_div_4():
    seed, frame, sid = 0x0123456789abcdef, (5 << 32) | 7, 3
    m = keep_mask(seed, frame, sid, 3, 6)
    g = 2
    for p in range(3):
        for c in range(6):
            words = philox4x32_10(p * g + c // 4, sid, frame & F32, frame >> 32, seed & F32, seed >> 32)
            assert m[p, c] == bool(int(words[c % 4]) & 1)


def test_keep_fraction_is_one_half():
    n_pix, c_out = 250000, 4
    m = keep_mask(0x5eed5eed12345678, (1 << 32) + 3, 9, n_pix, c_out)
    n = m.size
    assert n == 10 ** 6
    assert abs(m.sum() - n / 2) <= 6 * np.sqrt(n / 4)


def test_every_part_of_the_state_changes_the_mask():
    seed, frame, sid = 0x0123456789abcdef, (5 << 32) | 7, 17
    base = keep_mask(seed, frame, sid, 300, 64)
    variants = {'seed low word': (seed ^ 1, frame, sid), 'seed high word': (seed ^ (1 << 40), frame, sid),
                'frame low word': (seed, frame + 1, sid), 'frame high word': (seed, frame + (1 << 32), sid),
                'stream id': (seed, frame, sid + 1)}
    for name, args in variants.items():
        other = keep_mask(*args, 300, 64)
        assert 0.4 < (other != base).mean() < 0.6, name  # an independent draw, not a shifted copy


def test_negative_int64_seed_is_the_same_64_bits():
    seed = -0x1234567890abcdef
    assert np.array_equal(keep_mask(seed, 2, 1, 40, 12), keep_mask(seed + 2 ** 64, 2, 1, 40, 12))


def test_ragged_channel_groups_do_not_alias_the_next_pixel():
    """c_out % 4 != 0: the last, partial group of pixel p has its own counter, not that of group 0 of pixel p + 1 (with
    c_out < 4 that aliasing would give every pixel one mask)."""
    for c_out in (1, 2, 3, 5, 6, 30):
        m = keep_mask(0xfeedface0badcafe, (2 << 32) | 11, 5, 4096, c_out)
        last, r = c_out // 4 * 4, c_out % 4
        same = (m[:-1, last:last + r] == m[1:, :r]).mean()
        assert 0.45 < same < 0.55, c_out
        assert 0.45 < m.mean() < 0.55


def test_set_dropout_refuses_a_null_layer_without_device():
    lib = _lib.load()
    assert lib.ojf_segconv_set_dropout(None, None, 0, 0) != 0 and b'null' in lib.ojf_last_error()
    assert lib.ojf_segconv_set_dropout(None, None, 0, 1) != 0
