"""The word-wise steps of the two shift registers behind the scrambling sequence (openlte_amd/csrc/gold_run.h: gold_step_x1, gold_step_x2),
restated in Python, against the bitwise definition of 36.211 7.2.  Words are LSB-first: bit n & 31 of word n >> 5.  The PDSCH demodulators
take one word per run from the basis tables and step the rest; tests/test_gold_run_gpu.py holds the kernels against the table method."""
import numpy as np
import pytest

M32 = 0xFFFFFFFF
N_WORDS = 400  # a few hundred words each; the longest allocation (100 PRB, 64QAM, CFI 1) takes 2 926


def step_x1(W):
    T = (W >> 1) ^ (W >> 4)
    L = T & 15
    return (T ^ ((L & 1) << 31) ^ (L << 28)) & M32


def step_x2(W):
    T = (W >> 1) ^ (W >> 2) ^ (W >> 3) ^ (W >> 4)
    L = T & 15
    return (T ^ (L << 28) ^ (L << 29) ^ (L << 30) ^ (L << 31)) & M32


def bitwise(c_init, n_bits):
    """x1(1600 ...), x2(1600 ...) of 36.211 7.2, bit by bit"""
    n = 1600 + n_bits
    x1, x2 = [1] + [0] * 30, [(c_init >> i) & 1 for i in range(31)]
    for i in range(n - 31):
        x1.append(x1[i + 3] ^ x1[i])
        x2.append(x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i])
    return np.array(x1[1600:], np.uint8), np.array(x2[1600:], np.uint8)


def words(bits):
    return [int(w) for w in np.packbits(bits, bitorder="little").view("<u4")]


def stepped(w0, step, n):
    out = [w0]
    for _ in range(n - 1):
        out.append(step(out[-1]))
    return out


RNG = np.random.default_rng(36211)
C_INITS = [int(c) for c in RNG.integers(1, 2 ** 31, 24)] + [1 << b for b in range(31)] + [2 ** 31 - 1, 0,
           (0xFFFF << 14 | 9 << 9 | 503) & 0x7FFFFFFF, 1 << 14]  # random 31-bit values, one set bit, all bits, none, the RNTI / subframe / cell extremes


@pytest.fixture(scope="module")
def x1_words():
    return words(bitwise(0, 32 * N_WORDS)[0])


def test_x1_step(x1_words):
    assert stepped(x1_words[0], step_x1, N_WORDS) == x1_words
    for w0 in (1, 7, 123, N_WORDS - 2):  # from any word of the sequence, as a run does
        assert stepped(x1_words[w0], step_x1, N_WORDS - w0) == x1_words[w0:]


@pytest.mark.parametrize("c_init", C_INITS)
def test_x2_step_and_the_scrambling_words(c_init, x1_words):
    x1b, x2b = bitwise(c_init, 32 * N_WORDS)
    x2w = words(x2b)
    assert stepped(x2w[0], step_x2, N_WORDS) == x2w
    # runs of 2, 4 and 8 words the way gold_fill_words forms them: both registers' words at the run's first word, the rest stepped
    c = words(x1b ^ x2b)
    for R in (2, 4, 8):
        got = []
        for w0 in range(0, N_WORDS, R):
            got += [a ^ b for a, b in zip(stepped(x1_words[w0], step_x1, R), stepped(x2w[w0], step_x2, R))]
        assert got == c, R


def test_steps_are_linear():
    """What lets a run start from the XOR of basis-table words: step(a ^ b) = step(a) ^ step(b), on arbitrary words"""
    for a, b in RNG.integers(0, 2 ** 32, (200, 2)):
        a, b = int(a), int(b)
        assert step_x1(a ^ b) == step_x1(a) ^ step_x1(b) and step_x2(a ^ b) == step_x2(a) ^ step_x2(b)
