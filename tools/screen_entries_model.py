"""CPU model (numpy, no GPU) of how many rows the screening kernel appends per query, by bucket rule and exchange cadence.

``python tools/screen_entries_model.py`` prints the table of profiles/bound_exchange/README.md.  The model, per query:

* 1 M iid scores N(0, 1 / 384) (unit vectors in 384 dimensions), cut into 4 slices that advance in lockstep, 384 rows
  per slice and round (twelve waves, one 32-row tile each);
* every slice keeps a top-10 pool of its own rows (empty at the start of the slice phase) and appends every row that
  reaches ``bound - band``, band = 0.005, where ``bound`` is the best lower bound of the 10th best score it knows: the
  10th best of a 2 048-row sample, its pool's minimum once the pool is full, and what the last exchange gave it;
* the buckets (row id mod B) are seeded by the sample and fed by the rows the pools accept; at an exchange round a slice
  publishes its own bound to ``tau`` and takes the larger of ``tau`` and the buckets' bound - the MINIMUM of the B
  buckets (the rule the kernel had with B = 10) or the 10th LARGEST of them.

Left out: the fp16 copies of the bounds in registers and their 8-tile refresh, the first tile's single offer, waves of
a slice at different rounds, and everything about time.  The kernel therefore appends more than the model; the model
is for the RATIO between rules and cadences.
"""
import numpy as np

NQ, N, SLICES, ROUND_ROWS, K, SAMPLE, BAND = 24, 1_000_000, 4, 384, 10, 2_048, 0.005
NEG = np.float32(-np.inf)


def schedule(name, rounds):
    r = np.arange(rounds)
    if name == "never":
        return np.zeros(rounds, bool)
    if name == "0, 16, every 64":
        return (r == 0) | (r == 16) | (r % 64 == 0)
    if name == "0, 1, 2, 4, 8, every 16":
        return np.isin(r, (0, 1, 2, 4, 8)) | (r % 16 == 0)
    if name == "every 4":
        return r % 4 == 0
    raise ValueError(name)


def bucket_bound(buckets, rule):
    """[NQ][B] bucket maxima -> [NQ] bound (-inf: none)"""
    if rule == "min":
        return buckets.min(axis=1)
    b = buckets.shape[1]
    return np.partition(buckets, b - K, axis=1)[:, b - K]


def appended_per_query(scores, n_buckets, rule, cadence):
    per_slice = N // SLICES
    rounds = per_slice // ROUND_ROWS
    exchange = schedule(cadence, rounds)
    sample = scores[:, :SAMPLE]
    sample_bound = np.partition(sample, SAMPLE - K, axis=1)[:, SAMPLE - K]
    buckets = np.full((NQ, n_buckets), NEG, np.float32)
    ids = np.arange(SAMPLE) % n_buckets
    for b in range(n_buckets):
        buckets[:, b] = sample[:, ids == b].max(axis=1)
    pool = np.full((NQ, SLICES, K), NEG, np.float32)
    bound = np.repeat(sample_bound[:, None], SLICES, axis=1)            # [NQ][SLICES]
    tau = sample_bound.copy()
    appended = np.zeros(NQ, np.int64)
    qi = np.arange(NQ)[:, None, None]
    for r in range(rounds):
        if exchange[r] and n_buckets:
            tau = np.maximum(tau, bound.max(axis=1))
            bound = np.maximum(bound, np.maximum(tau, bucket_bound(buckets, rule))[:, None])
        lo = np.arange(SLICES)[:, None] * per_slice + r * ROUND_ROWS + np.arange(ROUND_ROWS)[None, :]   # row ids
        x = scores[:, lo]                                                                               # [NQ][SLICES][ROUND_ROWS]
        appended += (x >= (bound - BAND)[:, :, None]).sum(axis=(1, 2))
        accepted = x > pool.min(axis=2)[:, :, None]
        if n_buckets and accepted.any():
            q, s, j = np.nonzero(accepted)
            np.maximum.at(buckets, (q, lo[s, j] % n_buckets), x[q, s, j])
        both = np.concatenate([pool, x], axis=2)
        pool = np.partition(both, both.shape[2] - K, axis=2)[:, :, -K:]
        bound = np.maximum(bound, pool.min(axis=2))                    # (-inf while the pool is not full)
    return appended.mean()


def main():
    rng = np.random.default_rng(384)
    scores = (rng.standard_normal((NQ, N), dtype=np.float32) / np.float32(np.sqrt(384.0))).astype(np.float32)
    kth = np.partition(scores, N - K, axis=1)[:, N - K]
    print(f"rows inside the band of the true 10th best: {(scores >= (kth - BAND)[:, None]).sum(axis=1).mean():.0f} per query")
    cadences = ("0, 16, every 64", "0, 1, 2, 4, 8, every 16", "every 4")
    print("| buckets, rule | " + " | ".join(cadences) + " |")
    print("|---|" + "---|" * len(cadences))
    for n_buckets, rule, label in ((10, "min", "10, minimum"), (16, "kth", "16, 10th largest"), (32, "kth", "32, 10th largest"),
                                   (64, "kth", "64, 10th largest")):
        cells = [f"{appended_per_query(scores, n_buckets, rule, c):.0f}" for c in cadences]
        print(f"| {label} | " + " | ".join(cells) + " |", flush=True)
    print(f"| no exchange at all | {appended_per_query(scores, 10, 'min', 'never'):.0f} | | |")


if __name__ == "__main__":
    main()
