"""GPU: the three max-log-MAP modes (MI_LTE_TURBO_BCJR, _BCJR_EARLY, _BCJR_BLOCK) against their plain-C models at EVERY one of the 188
block sizes, not the handful tests/test_bcjr_gpu.py samples.  The kernels have paths that depend on K: k_bcjr_half cuts a block into
8 / 4 / 2 / 1 segments (bcjr_n_seg) with an alpha hand-over between them and, where K < kpad64(K), a last segment that ends short;
k_bcjr_block runs 32 / 64 / 96 steps per lane on 2 .. 64 lanes with a short last lane.  The inputs include what the Gaussian code words
of the other file never reach: the +-127 rails and non-code-word values, where the path metrics are widest and the packed-int16
arithmetic (no saturation: it rests on the model's range claim, tests/test_oracle.py) has the least room."""
import os

import numpy as np
import pytest

import lte_testdata as td
from test_bcjr_gpu import llr_blocks

pytestmark = pytest.mark.gpu

# input kinds: AWGN near the decoding threshold (sigma 0.9 in llr_blocks' convention), a code word at +-127 with ~2 % flips, and two
# that are no code word at all: uniform int8 in [-127, 127], and +-127 with random signs (lte_testdata.turbo_blocks)
KINDS = ("awgn0.9", "hard127", "noise", "rand127")
CODE_WORD_KINDS = ("awgn0.9", "hard127")
UNIQ = 8  # distinct blocks per size: two of each kind, block u is of kind KINDS[u % 4]
BATCH_ITERS = ((8, False), (3, True))  # (iterations, 3GPP-exact interleaver): as tests/test_bcjr_gpu.py
BLOCK_ITERS = ((8, False), (2, True))
HOST_THREADS = max(1, min(16, len(os.sched_getaffinity(0))))


def mixed_blocks(port, K, uniq, seed):
    """uniq blocks of size K, kind KINDS[u % 4] -> (tx [uniq, K], soft int8 [uniq, 3 (K + 4)], kind index per block)."""
    per = -(-uniq // len(KINDS))
    tx = np.zeros((uniq, K), np.uint8)
    soft = np.zeros((uniq, 3 * (K + 4)), np.int8)
    kind = np.arange(uniq) % len(KINDS)
    for k, name in enumerate(KINDS):
        if name.startswith("awgn"):
            t, s = llr_blocks(port, K, per, float(name[4:]), seed=seed + k)
        else:
            t, s = td.turbo_blocks(port, K, per, name, seed=seed + k)
        rows = np.flatnonzero(kind == k)
        tx[rows], soft[rows] = t[:len(rows)], s[:len(rows)].astype(np.int8)
    return tx, soft, kind


def model_decode(model, soft, K, n_iter, spec):
    out = np.zeros((soft.shape[0], K), np.uint8)
    for b in range(soft.shape[0]):
        model(np.ascontiguousarray(soft[b].astype(np.int16)), K, n_iter, 1 if spec else 0, out[b])
    return out


def replicate(n_cb, uniq):
    """The fixed index pattern of test_bcjr_full_batch_property: every unique block in every tile, at shifting lanes."""
    i = np.arange(n_cb)
    return (i * 5 + i // 64) % uniq


def test_bcjr_all_188_block_sizes_bit_exact_vs_the_models(ctx, port):
    """Every size x {batch kernels, one block per wavefront} x {wrapped interleaver x 8 iterations, 3GPP interleaver x 3 (2)} x four input
    kinds.  Batch kernels: 130 code blocks = three tiles, the last one ragged, so the last pair's second half is empty (the odd-tile
    branch of mi_turbo_bcjr_begin and the duplicated last tile of k_bcjr_half); every block of every tile is a replica of one of
    UNIQ model-decoded blocks.  One run reports every failing (K, mode, interleaver, kind)."""
    import openlte_amd as m
    assert len(td.ALL_K) == 188
    n_batch = 130
    idx = replicate(n_batch, UNIQ)

    def case(K):
        tx, soft, kind = mixed_blocks(port, K, UNIQ, seed=7 * K)
        want = {("batch", it): model_decode(port.lo_turbo_decode_bcjr, soft, K, *it) for it in BATCH_ITERS}
        want.update({("block", it): model_decode(port.lo_turbo_decode_bcjr_block, soft, K, *it) for it in BLOCK_ITERS})
        return K, tx, soft, kind, want

    bad, undecoded, n_checked = [], [], 0
    for c0 in range(0, len(td.ALL_K), 32):  # the models of 32 sizes at a time on the host cores, then those sizes on the GPU
        for K, tx, soft, kind, want in td.parallel_map(case, td.ALL_K[c0:c0 + 32], threads=HOST_THREADS):
            big = np.ascontiguousarray(soft[idx])
            for (name, it), w in want.items():
                n_iter, spec = it
                if name == "batch":
                    got, w, kd, t = ctx.turbo_decode(big, K, mode=m.TURBO_BCJR, n_iter=n_iter, qpp_spec=spec), w[idx], kind[idx], tx[idx]
                else:
                    got, kd, t = ctx.turbo_decode(soft, K, mode=m.TURBO_BCJR_BLOCK, n_iter=n_iter, qpp_spec=spec), kind, tx
                assert got.shape == w.shape
                wrong = (got != w).any(axis=1)
                for k, kname in enumerate(KINDS):
                    n_checked += 1
                    if wrong[kd == k].any():
                        bad.append((K, name, int(spec), kname, int(wrong[kd == k].sum())))
                    # the decoder decodes: code words, 8 iterations, wherever the wrapped interleaver is a permutation
                    if kname in CODE_WORD_KINDS and not spec and K not in td.OVERFLOW_K and (got[kd == k] != t[kd == k]).any():
                        undecoded.append((K, name, kname, int((got[kd == k] != t[kd == k]).any(axis=1).sum())))
    assert n_checked == 188 * 2 * 2 * 4
    assert not bad, "%d (K, mode, spec, kind, n_blocks) differing from the model: %s" % (len(bad), bad[:60])
    assert not undecoded, "code words not decoded to the transmitted bits (K, mode, kind, n_blocks): %s" % undecoded[:40]


# one size of each (n_seg, ragged) class of k_bcjr_half: (2, ragged with 16 / 32 steps missing), (4, ragged), (4, full), (8, full), (1, long)
SHAPE_K = (1008, 1120, 2016, 2304, 5632, 5824)


def test_bcjr_batch_shapes_after_a_large_decode(ctx, port):
    """n_cb = 1, one and two full tiles, 65 (a full tile + one block), 192 (three full tiles: only the odd-tile branch) at one size of each
    segment class.  Immediately before each of them the same context decodes 256 blocks of K = 6144 at the rails, which leaves every
    scratch array the small decode will lay out full of stale values: a lane past the batch end must not see them."""
    import openlte_amd as m
    import ctypes as C
    port.lo_bcjr_n_seg.restype = C.c_uint32
    assert [(int(port.lo_bcjr_n_seg(K)), K % 64 != 0) for K in SHAPE_K] == [(2, True), (2, True), (4, True), (4, False), (8, False), (1, False)]
    Kb, nb = 6144, 256
    _, sb = td.turbo_blocks(port, Kb, 4, "rand127", seed=1)
    d_big, d_big_out = ctx.to_device(sb[replicate(nb, 4)]), ctx.alloc(nb * Kb)
    bad = []
    try:
        for K in SHAPE_K:
            tx, soft, kind = mixed_blocks(port, K, UNIQ, seed=11 * K)
            for n_iter, spec in BATCH_ITERS:
                want = model_decode(port.lo_turbo_decode_bcjr, soft, K, n_iter, spec)
                for n_cb in (1, 64, 65, 128, 192):
                    idx = (replicate(n_cb, UNIQ) + n_cb) % UNIQ  # (n_cb = 1 is then not always block 0)
                    ctx.turbo_decode_dev(d_big, m.SOFT_I8, Kb, nb, d_big_out, mode=m.TURBO_BCJR, n_iter=2)
                    got = ctx.turbo_decode(soft[idx], K, mode=m.TURBO_BCJR, n_iter=n_iter, qpp_spec=spec)
                    wrong = (got != want[idx]).any(axis=1)
                    if wrong.any():
                        bad.append((K, n_cb, int(spec), int(wrong.sum()), np.flatnonzero(wrong)[:4].tolist()))
    finally:
        d_big.free(); d_big_out.free()
    assert not bad, "(K, n_cb, spec, n_blocks, first blocks) differing from the model: %s" % bad


@pytest.mark.parametrize("K,spec,n", [(1008, False, 4 * 128 - 37), (2304, True, 3 * 128 + 64 - 37), (4096, False, 4 * 128 - 37)])
def test_bcjr_early_termination_at_the_segment_classes(ctx, port, K, spec, n):
    """The scheme of test_bcjr_early_termination_is_the_model_at_the_iterations_each_pair_ran at n_seg = 2 with a short last segment
    (1008), 4 (2304; 411 blocks: an odd tile count, the last pair's second half empty) and 8 (4096).  A stopped pair's segments all return
    at once and its alpha / beta boundary buffers stay what its last iteration wrote.  Every block of every pair: the output equals the
    model run for the iterations the pair reports, and the stopping rule is re-derived on the model from iteration 1 on -- no iteration
    before the last changed nothing, and (unless all 8 ran) the last one did."""
    import openlte_amd as m
    n_pairs = (n + 127) // 128
    sig = np.concatenate([np.full(128, 0.3), np.full(128, 0.85), np.full(128, 1.05), np.full(n - 384, 0.6)])
    sig[2 * 128 + 5] = 2.5  # one hopeless block keeps its pair iterating
    seeds = [1000 * K + b for b in range(n)]
    made = td.parallel_map(lambda b: llr_blocks(port, K, 1, float(sig[b]), seed=seeds[b]), range(n), threads=HOST_THREADS)
    tx, soft = np.concatenate([t for t, _ in made]), np.concatenate([s for _, s in made])
    got = ctx.turbo_decode(soft, K, mode=m.TURBO_BCJR_EARLY, n_iter=8, qpp_spec=spec)
    iters = ctx.turbo_early_exit_iterations()
    print("K = %d: iterations per pair %s" % (K, iters.tolist()))
    assert len(iters) == n_pairs and iters.min() >= 2 and iters.max() <= 8
    assert iters[0] == 2 and iters[2] == 8 and iters[1] <= 6, iters  # the three qualities: clean, moderate, one block below threshold
    full = ctx.turbo_decode(soft, K, mode=m.TURBO_BCJR, n_iter=8, qpp_spec=spec)
    i16 = soft.astype(np.int16)

    def decisions(job):
        b, k = job
        out = np.zeros(K, np.uint8)
        port.lo_turbo_decode_bcjr(np.ascontiguousarray(i16[b]), K, k, 1 if spec else 0, out)
        return out

    for p in range(n_pairs):
        blk = np.arange(128 * p, min(n, 128 * p + 128))
        last = int(iters[p])
        jobs = [(int(b), k) for k in range(1, last + 1) for b in blk]
        dec = np.stack(td.parallel_map(decisions, jobs, threads=HOST_THREADS)).reshape(last, len(blk), K)  # dec[k - 1]: after k iterations
        assert (got[blk] == dec[last - 1]).all(), (p, last, int((got[blk] != dec[last - 1]).any(axis=1).sum()))
        for k in range(2, last):  # the pair did not stop earlier: each of those iterations changed a decision
            assert (dec[k - 1] != dec[k - 2]).any(), (p, last, k)
        if last < 8:
            assert (dec[last - 1] == dec[last - 2]).all(), (p, last)
        ok = sig[blk] < 2
        assert (got[blk][ok] == tx[blk][ok]).all() and (got[blk][ok] == full[blk][ok]).all()  # stopping early costs nothing on blocks that decode
