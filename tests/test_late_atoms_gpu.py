"""The MaxSim tile engine held to equality on the MI355X (tests/late_atoms_cases.py has the world and the restatement).

The atoms - every query token against every document token, each as a one-token query and a one-token document through
``sskd_late_rerank`` - are taken once; then the raw scores of ``sskd_late_rerank``, the scores and the argmax of
``sskd_latet_maxsim_fwd``, the raw scores of ``sskd_latec_rerank`` (2 and 4 bits, on a store written by
``sskd_latec_compress``) and ``S`` of ``sskd_plaid_centroid_scores`` must equal the NumPy restatement bit for bit."""
import numpy as np
import pytest
import torch

import late_atoms_cases as ac
import late_codec_cases as cc
from capi_helpers import stream

pytestmark = pytest.mark.gpu


def _dev(a: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(a).cuda()


def _rerank_raw(lib, q_bits, q_lims, d_bits, d_lims, cand, k):
    """``sskd_late_rerank`` with ``d_out_raw``: the raw scores ``[nq, R]``."""
    nq, R_ = cand.shape
    q_lims = np.ascontiguousarray(q_lims, np.int64)
    keep = (_dev(q_bits), _dev(q_lims), _dev(d_bits), _dev(np.ascontiguousarray(d_lims, np.int64)), _dev(cand))
    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    raw = torch.full((nq, R_), 7.0, dtype=torch.float32, device="cuda")
    rc = lib.sskd_late_rerank(keep[0].data_ptr(), q_lims.ctypes.data, keep[1].data_ptr(), nq, keep[2].data_ptr(), keep[3].data_ptr(),
                              len(d_lims) - 1, int(d_lims[-1]), keep[4].data_ptr(), R_, k, 0, D.data_ptr(), I.data_ptr(),
                              raw.data_ptr(), None, 0, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.sskd_last_error()
    return raw.cpu().numpy()


def _atoms(lib, q_bits, d_bits) -> np.ndarray:
    n_q, n_d = q_bits.shape[0], d_bits.shape[0]
    out = np.empty((n_q, n_d), dtype=np.float32)
    for lo, hi, cand in ac.atom_requests(n_q, n_d):
        out[:, lo:hi] = _rerank_raw(lib, q_bits, np.arange(n_q + 1), d_bits, np.arange(n_d + 1), cand, hi - lo)
    assert np.isfinite(out).all()
    return out


class Compressed:
    """The world's documents compressed by ``sskd_latec_compress``; the atoms of the decoded rows."""

    def __init__(self, lib, w: ac.World, nbits: int):
        cen, cut, wts = w.codec[nbits]
        n = w.d_bits.shape[0]
        self.nbits, self.C = nbits, cen.shape[0]
        self.cen, self.wts = _dev(cen), _dev(wts)
        self.cid = torch.empty(n, dtype=torch.int32, device="cuda")
        self.scale = torch.empty(n, dtype=torch.float32, device="cuda")
        self.codes = torch.empty((n, 48 * nbits), dtype=torch.uint8, device="cuda")
        keep = (_dev(w.d_bits), _dev(cc.assign_rows(w.d_bits, cen)), _dev(cut))
        rc = lib.sskd_latec_compress(keep[0].data_ptr(), keep[1].data_ptr(), n, self.cen.data_ptr(), self.C, keep[2].data_ptr(),
                                     self.wts.data_ptr(), nbits, self.cid.data_ptr(), self.scale.data_ptr(), self.codes.data_ptr(),
                                     0, n, stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.sskd_last_error()
        self.scale_host = self.scale.cpu().numpy()
        dec = cc.decode_rows(self.cid.cpu().numpy(), self.codes.cpu().numpy(), cen, wts, nbits)
        self.atoms = _atoms(lib, w.q_bits, dec)


@pytest.fixture(scope="module")
def world(gpu, native_lib):
    """The world and its atoms, taken once and left unchanged."""
    w = ac.World()
    w.atoms = _atoms(native_lib, w.q_bits, w.d_bits)
    w.compressed = {nbits: Compressed(native_lib, w, nbits) for nbits in (2, 4)}
    w.centroid_atoms = _atoms(native_lib, w.q_bits, w.codec[2][0])
    return w


def test_rerank_raw_scores_are_the_restated_bits(native_lib, world):
    for b, pool in enumerate(ac.BATCHES):
        q_bits, q_lims, cand = world.batch(b)
        want, _ = ac.maxsim(world.atoms, world.q_lims, pool, world.d_lims, cand)
        got = _rerank_raw(native_lib, q_bits, q_lims, world.d_bits, world.d_lims, cand, 1)
        assert ac.same_bits(got, want), f"batch {pool}"


def test_training_forward_scores_and_argmax_are_the_restated_bits(native_lib, world):
    lib = native_lib
    d_tok, d_lims = _dev(world.d_bits), _dev(world.d_lims)
    for b, pool in enumerate(ac.BATCHES):
        q_bits, q_lims, cand = world.batch(b)
        want, want_arg = ac.maxsim(world.atoms, world.q_lims, pool, world.d_lims, cand)
        nq, stride = len(pool), want_arg.shape[2]
        keep = (_dev(q_bits), _dev(q_lims), _dev(cand))
        scores = torch.full((nq, ac.R), 7.0, dtype=torch.float32, device="cuda")
        arg = torch.full((nq, ac.R, stride), -7, dtype=torch.int32, device="cuda")
        rc = lib.sskd_latet_maxsim_fwd(keep[0].data_ptr(), q_lims.ctypes.data, keep[1].data_ptr(), nq, int(q_lims[-1]),
                                       d_tok.data_ptr(), d_lims.data_ptr(), len(world.d_lims) - 1, int(world.d_lims[-1]),
                                       keep[2].data_ptr(), ac.R, scores.data_ptr(), arg.data_ptr(), stride, stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.sskd_last_error()
        assert ac.same_bits(scores.cpu().numpy(), want), f"batch {pool}: scores"
        assert np.array_equal(arg.cpu().numpy(), want_arg), f"batch {pool}: argmax"


@pytest.mark.parametrize("nbits", [2, 4])
def test_compressed_raw_scores_are_the_restated_bits(native_lib, world, nbits):
    lib, st = native_lib, world.compressed[nbits]
    d_lims = _dev(world.d_lims)
    for b, pool in enumerate(ac.BATCHES):
        q_bits, q_lims, cand = world.batch(b)
        want, _ = ac.maxsim(st.atoms, world.q_lims, pool, world.d_lims, cand, scale=st.scale_host)
        nq = len(pool)
        keep = (_dev(q_bits), _dev(q_lims), _dev(cand))
        D = torch.empty((nq, 1), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, 1), dtype=torch.int64, device="cuda")
        raw = torch.full((nq, ac.R), 7.0, dtype=torch.float32, device="cuda")
        rc = lib.sskd_latec_rerank(keep[0].data_ptr(), q_lims.ctypes.data, keep[1].data_ptr(), nq, st.cid.data_ptr(),
                                   st.scale.data_ptr(), st.codes.data_ptr(), nbits, st.cen.data_ptr(), st.C, st.wts.data_ptr(),
                                   d_lims.data_ptr(), len(world.d_lims) - 1, int(world.d_lims[-1]), keep[2].data_ptr(), ac.R, 1, 0,
                                   D.data_ptr(), I.data_ptr(), raw.data_ptr(), None, 0, stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.sskd_last_error()
        assert ac.same_bits(raw.cpu().numpy(), want), f"batch {pool}"


@pytest.mark.parametrize("n_centroids", ac.CENTROIDS)
def test_centroid_scores_are_the_atoms(native_lib, world, n_centroids):
    lib = native_lib
    T = world.q_bits.shape[0]
    q, cen = _dev(world.q_bits), _dev(world.codec[2][0][:n_centroids])
    S = torch.full((n_centroids, T), 7.0, dtype=torch.float32, device="cuda")
    rc = lib.sskd_plaid_centroid_scores(q.data_ptr(), T, cen.data_ptr(), n_centroids, S.data_ptr(), T, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.sskd_last_error()
    assert ac.same_bits(S.cpu().numpy(), world.centroid_atoms[:, :n_centroids].T)
