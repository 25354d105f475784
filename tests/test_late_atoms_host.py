"""The restatement of tests/late_atoms_cases.py on the CPU (no GPU, no library): fed with the fp64 dot products rounded
to fp32 in place of the device's atoms, its scores lie inside the derived bands of the fp64 references and its argmax
is the fp64 one wherever that is decided by more than the rounding."""
import numpy as np

import late_atoms_cases as ac
import late_cases as lc
import late_codec_cases as cc


def _in_band(raw, ref, cand):
    want = ref.of_candidates(ref.s64, cand)
    E = ref.of_candidates(ref.E, cand, fill=0.0)
    absent = np.isneginf(want)
    assert np.array_equal(np.isneginf(raw), absent)
    assert (np.abs(raw[~absent].astype(np.float64) - want[~absent]) <= E[~absent]).all()


def test_world_reaches_every_branch():
    w = ac.World()
    assert [ac.stride_of([ac.TQS[k] for k in pool]) // 32 for pool in ac.BATCHES] == [1, 1, 2, 3, 4]
    assert max(len(pool) for pool in ac.BATCHES) == 5 and all(c.shape == (len(p), ac.R) for c, p in zip(w.cand, ac.BATCHES))
    for cand in w.cand:
        assert ((cand == -1).sum(axis=1) == 1).all() and ((cand == ac.EMPTY_ROW).sum(axis=1) == 1).all()
    calls = list(ac.atom_requests(3, 2500))
    assert [(lo, hi) for lo, hi, _ in calls] == [(0, 1024), (1024, 2048), (2048, 2500)]
    assert calls[2][2].shape == (3, 452) and calls[2][2][1, 0] == 2048


def test_restated_scores_lie_within_the_fp64_band():
    w = ac.World()
    atoms = ac.host_atoms(w.q_bits, w.d_bits)
    for b, pool in enumerate(ac.BATCHES):
        q_bits, q_lims, cand = w.batch(b)
        raw, arg = ac.maxsim(atoms, w.q_lims, pool, w.d_lims, cand)
        _in_band(raw, lc.Reference(q_bits, q_lims, w.d_bits, w.d_lims), cand)
        # the argmax: the smallest index that holds the maximum of the atoms
        for q, k in enumerate(pool):
            for c, row in enumerate(cand[q]):
                a = arg[q, c]
                if row < 0 or row == ac.EMPTY_ROW:
                    assert (a == -1).all()
                    continue
                block = atoms[w.q_lims[k]: w.q_lims[k + 1], w.d_lims[row]: w.d_lims[row + 1]]
                tq = block.shape[0]
                assert (a[tq:] == -1).all() and (a[:tq] >= 0).all() and (a[:tq] < block.shape[1]).all()
                for i in range(tq):
                    assert block[i, a[i]] == block[i].max() and not (block[i, : a[i]] == block[i].max()).any()
    # the planted ties resolve to the smaller index, the planted best tokens sit in the last partial tile
    raw, arg = ac.maxsim(atoms, w.q_lims, (1, 2, 3, 4), w.d_lims, np.array([[2], [3], [4], [5]], np.int64))
    assert arg[0, 0, 3] == 5 and arg[1, 0, 0] == 32 and arg[2, 0, 40] == 64 and arg[3, 0, 100] == 10


def test_restated_compressed_scores_lie_within_the_fp64_band():
    w = ac.World()
    for nbits in (2, 4):
        cen, cut, wts = w.codec[nbits]
        cid, scale, codes, dec = cc.compress_rows(w.d_bits, cc.assign_rows(w.d_bits, cen), cen, cut, wts, nbits)
        assert np.array_equal(dec, cc.decode_rows(cid, codes, cen, wts, nbits))
        atoms = ac.host_atoms(w.q_bits, dec)
        for b, pool in enumerate(ac.BATCHES):
            q_bits, q_lims, cand = w.batch(b)
            raw, _ = ac.maxsim(atoms, w.q_lims, pool, w.d_lims, cand, scale=scale)
            _in_band(raw, cc.ReferenceC(q_bits, q_lims, dec, scale, w.d_lims), cand)
