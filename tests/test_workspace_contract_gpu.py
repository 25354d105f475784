"""The workspace contract on the MI355X: every workspace-taking entry point on poisoned, guarded scratch memory.

``include/sskd_amd.h`` (conventions block): a workspace may hold anything on entry, nothing outside the reported size is
touched, contents on return are unspecified.  DESIGN.md "Workspace contract" lists every sub-buffer of every carve with
its first writer and its readers; this module is the detector for what a refactor may lose.

``test_workspace_contract``: ``workspace_cases.CASES`` x shapes x ``FILLS``.  Each run gets a workspace of EXACTLY the
bytes its size query reports, between two guard regions, holding 0x00, 0xFF, 0x7F or what the same entry point left
behind on a larger-scoring world.  After a synchronise: the guards are intact, the shape's reference assertion holds (the
one the entry point's own test makes), and - for bit-deterministic entry points - the outputs equal the 0x00 run bit for
bit.  A failure names the entry point, the shape, the fill and the first differing output element.

The second half runs the Python layer's shared buffers the way a serving process does: ONE index through its one-pass,
chained, range, grouped and screened searches in turn, each step compared bit for bit with the same call on a freshly
built index, then again with the shared buffer swapped for an oversized poisoned one before every step.  The same for the
late-interaction index (exact, then compressed re-rank) and the encoder's shared workspace across two batch shapes.
"""
import numpy as np
import pytest
import torch

import workspace_cases as wc

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
_baseline = {}   # (entry, shape) -> (outputs of the 0x00 run, its problems)

TRIPLES = [(entry, shape, fill) for entry, shape in wc.all_runs() for fill in wc.FILLS]


def _zero_run(lib, entry, shape, run):
    key = (entry, shape.name)
    if key not in _baseline:
        _baseline[key] = _check(lib, entry, shape, run, 0x00, None)
    return _baseline[key]


def _check(lib, entry, shape, run, fill, baseline):
    return wc.check_fill(entry, shape.name, fill, lambda g: run.run(lib, g.ptr, g.need), run.need, "cuda",
                         baseline=baseline, deterministic=shape.deterministic, reference=run.check,
                         prior=lambda g: run.prior(lib, g.ptr, g.need), sync=torch.cuda.synchronize, stable=run.stable,
                         expect_written=True)


@pytest.mark.parametrize("entry, shape, fill", TRIPLES,
                         ids=[f"{e.replace('sskd_', '').replace('_workspace_bytes', '')}-{s.name}-{wc.fill_name(f)}"
                              for e, s, f in TRIPLES])
def test_workspace_contract(gpu, native_lib, entry, shape, fill):
    run = wc.prepared(entry, shape, native_lib)
    base, problems = _zero_run(native_lib, entry, shape, run)
    if fill != 0x00:
        _, problems = _check(native_lib, entry, shape, run, fill, base)
    assert not problems, "\n".join(problems)


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer's shared buffers
# ---------------------------------------------------------------------------------------------------------------------
N_ROWS = 3001


def _same_bits(got, want, what):
    got = tuple(np.asarray(x) for x in (got if isinstance(got, tuple) else (got,)))
    want = tuple(np.asarray(x) for x in (want if isinstance(want, tuple) else (want,)))
    d = wc.first_difference(got, want)
    assert d is None, f"{what}: output {d[0]} differs from a fresh object's, first at element {d[1]}: {d[2]!r} != {d[3]!r}"


def _poisoned(nbytes, fill):
    return torch.full((int(nbytes),), fill, dtype=torch.uint8, device="cuda")


def _sequence(steps, fresh, subject, attr, what):
    """``steps``: (name, call(object)).  Reference: every step on its own freshly built object.  Then the steps in turn on
    ONE object, as they come; then again with the object's shared buffer ``attr`` replaced before every step by an
    oversized buffer of each byte fill, which the object must reuse."""
    want = []
    for name, call in steps:
        want.append(call(fresh(name)))
        torch.cuda.synchronize()
    obj = subject()
    for (name, call), ref in zip(steps, want):
        _same_bits(call(obj), ref, f"{what}: {name} after the steps before it")
    largest = getattr(obj, attr).numel()
    assert largest > 1
    for fill in wc.BYTE_FILLS:
        for (name, call), ref in zip(steps, want):
            buf = _poisoned(2 * largest + (1 << 20), fill)
            setattr(obj, attr, buf)
            got = call(obj)
            torch.cuda.synchronize()
            assert getattr(obj, attr) is buf, f"{what}: {name} did not reuse a buffer of {buf.numel()} bytes"
            _same_bits(got, ref, f"{what}: {name} on a shared buffer full of {wc.fill_name(fill)}")


def test_one_index_through_every_search_on_its_shared_workspace(gpu, native_lib):
    from semantic_search_kd_amd import FAISSIndexBuilder

    corpus, queries, _, _ = wc.world_arrays(N_ROWS)
    groups = [int(g) for g in np.arange(N_ROWS) // 3]
    thr = np.sort(queries[:5] @ corpus.T, axis=1)[:, -40].astype(np.float32)     # about 40 rows per query

    def build(_name=None):
        index = FAISSIndexBuilder(embedding_dim=wc.DIM, metric="ip", device=str(gpu))
        index.build_from_embeddings(corpus, groups=groups)
        assert index.screening
        return index

    def path(index, call, wanted):
        out = call(index)
        assert wanted(index.last_search_path), index.last_search_path
        return out

    steps = [
        ("one-pass nq 3", lambda ix: path(ix, lambda i: i.search(queries[:3], 10), lambda p: "onepass" in p)),
        ("chained nq 70 k 100", lambda ix: path(ix, lambda i: i.search(queries[:70], 100), lambda p: "screened" not in p and "onepass" not in p)),
        ("range_search", lambda ix: ix.range_search(queries[:5], thr)),
        ("search_grouped", lambda ix: path(ix, lambda i: i.search_grouped(queries[:33], 10), lambda p: p.startswith("grouped"))),
        ("screened nq 70 k 10", lambda ix: path(ix, lambda i: i.search(queries[:70], 10), lambda p: p.endswith("+screened"))),
        ("one-pass again", lambda ix: path(ix, lambda i: i.search(queries[:3], 10), lambda p: "onepass" in p)),
    ]
    _sequence(steps, build, build, "_workspace", "Index")


def test_one_late_index_through_exact_and_compressed_rerank(gpu, native_lib):
    import late_cases as lc
    import test_late_codec_gpu as tc
    import test_late_gpu as tl

    rng = np.random.default_rng(7600)
    tok, lims = lc.sweep_store()
    n = lims.size - 1
    codec = tc._codec(16, 2)
    q3, l3 = lc.queries(rng, [5, 33, 128])
    q2, l2 = lc.queries(rng, [64, 2])
    c100 = torch.from_numpy(lc.candidates(rng, 3, 100, n, must=lc.big_rows(lims)[:12])).cuda()
    c20 = torch.from_numpy(lc.candidates(rng, 2, 20, n)).cuda()

    def exact(_name=None):
        return tl._late(tok, lims, gpu)

    def compressed(late=None):
        late = exact() if late is None else late
        late.set_codec(*codec)
        late.compress()
        assert late.compressed
        return late

    def rerank(late, q, l, cand, k):
        D, I = late.rerank_device(q, l, cand, k)       # without the raw scores: they live in the workspace
        torch.cuda.synchronize()
        return D.cpu().numpy(), I.cpu().numpy()

    steps = [
        ("exact nq 3 R 100", lambda late: rerank(late, q3, l3, c100, 10)),
        ("compress, then compressed nq 3 R 100", lambda late: rerank(late if late.compressed else compressed(late), q3, l3, c100, 10)),
        ("compressed nq 2 R 20", lambda late: rerank(late if late.compressed else compressed(late), q2, l2, c20, 5)),
    ]
    # the poisoned rounds start from an object that is compressed already: they run the compressed steps, and the exact
    # step is covered by the plain round and by the C-ABI cases
    want = [call(exact()) for _, call in steps]
    late = exact()
    for (name, call), ref in zip(steps, want):
        _same_bits(call(late), ref, f"LateInteractionIndex: {name} after the steps before it")
    largest = late._workspace.numel()
    for fill in wc.BYTE_FILLS:
        for (name, call), ref in list(zip(steps, want))[1:]:
            buf = _poisoned(2 * largest + (1 << 20), fill)
            late._workspace = buf
            got = call(late)
            assert late._workspace is buf, name
            _same_bits(got, ref, f"LateInteractionIndex: {name} on a shared buffer full of {wc.fill_name(fill)}")
        fresh = exact()
        fresh._workspace = _poisoned(2 * largest + (1 << 20), fill)
        _same_bits(steps[0][1](fresh), want[0], f"LateInteractionIndex: {steps[0][0]} on a shared buffer full of {wc.fill_name(fill)}")


def test_one_encoder_across_two_batch_shapes_on_its_shared_workspace(gpu, native_lib):
    from oracle import encoder as enc_oracle
    from semantic_search_kd_amd import BertConfig, Mi355xSentenceEncoder

    cfg = BertConfig(num_hidden_layers=2)
    wide = enc_oracle.synthetic_token_ids(5, 100, seed=41, vocab=cfg.vocab_size, lengths=[100, 77, 33, 1, 64])
    short = enc_oracle.synthetic_token_ids(3, 40, seed=42, vocab=cfg.vocab_size, lengths=[40, 9, 2])

    def build(_name=None):
        return Mi355xSentenceEncoder.from_synthetic(cfg, device=str(gpu))

    def encode(enc, batch):
        out = enc.encode_token_ids(batch[0], batch[1], normalize=True)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    steps = [("5 x 100", lambda e: encode(e, wide)), ("3 x 40", lambda e: encode(e, short)), ("5 x 100 again", lambda e: encode(e, wide))]
    _sequence(steps, build, build, "_workspace", "Mi355xSentenceEncoder")
