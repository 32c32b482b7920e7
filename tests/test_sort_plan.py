"""Every branch of the sorted read's plan (sgx::sort_records), low key bytes included.

sort_records reads the keys' byte histograms and picks: a key window [lo, lo + kbits) below the
top varying byte, taken in chunks of <= 10 bits or as one segmented pass; a pass by the
partitioner or none; the on-chip bucket sort (k_bucket_sort), which gives up when a bucket
outgrows its halo; or LSD digit passes.  Each case below is an input built to reach one of those
branches.  Under flags = 0 it asserts the branch from ShuffleEngine.last_sort_plan(), so a case
that stops reaching its branch after a tuning change fails; the same input then runs, output
only, with the bucket path off (FLAG_NO_BUCKET_SORT), on the ballot-ranked kernels
(FLAG_ASSUME_LDS_DISORDER) and, for multi-partition reads, with the segmented passes off
(FLAG_NO_SEG_WINDOW).

Reference: plain numpy, not the oracle's reduce side -- np.argsort(kind="stable") on the signed
Longs, np.lexsort over the 10 key bytes; for R > 1 the partitions' members come from the
oracle's map side (map_write / canonical_reducer_sequences, as test_reduce_side._run) and each
partition's segment is the numpy stable sort of its canonical sequence.  Whole records are
compared bit-exactly; values and payloads carry the input position, so an unstable order shows.

The CPU test restates the plan's arithmetic (and the bucket sort's halo rule) in numpy and
checks that every case's input predicts the facts the GPU test asserts, so the inputs cannot
drift from their purpose unnoticed on a machine without a GPU."""
import functools

import numpy as np
import pytest

TILE = {16: 2048, 100: 512}  # k_bucket_sort's tile and halo (launch_bucket_sort)
HALO = {16: 255, 100: 127}
NAMES = ("path", "lo", "kbits", "window_passes", "digit_passes", "segmented", "use_p")


# ---------------------------------------------------------------- records ---------------
def _flip(u):
    """Unsigned order key (the sign-flipped Long the engine sorts by) -> the signed Long."""
    return (np.asarray(u, dtype=np.uint64) ^ np.uint64(1 << 63)).view(np.int64)


def _rec16(keys, base=0):
    """(Long, Long) records: value = input position (base + i)."""
    keys = np.asarray(keys, dtype=np.int64)
    a = np.empty((len(keys), 16), np.uint8)
    a[:, :8] = keys.astype("<i8").reshape(-1, 1).view(np.uint8)
    a[:, 8:] = (np.arange(len(keys), dtype="<i8") + base).reshape(-1, 1).view(np.uint8)
    return a


def _rec100(kb, base=0):
    """TeraSort records: 10 key bytes, then the input position (8 bytes) and a filler."""
    kb = np.asarray(kb, dtype=np.uint8)
    n = len(kb)
    a = np.empty((n, 100), np.uint8)
    a[:, :10] = kb
    a[:, 10:18] = (np.arange(n, dtype="<i8") + base).reshape(-1, 1).view(np.uint8)
    a[:, 18:] = (np.arange(82, dtype=np.uint8) * 3 + 1)[None, :]
    return a


def _spread(total, k):
    """total split over k buckets as evenly as integers allow."""
    return [total // k + (1 if i < total % k else 0) for i in range(k)]


def _top_byte_keys(counts, rng):
    """Longs whose sign-flipped top byte takes value b counts[b] times, low 56 bits random,
    in random order."""
    top = np.repeat(np.arange(len(counts), dtype=np.uint64), counts)
    u = (top << np.uint64(56)) | rng.integers(0, 1 << 56, size=len(top), dtype=np.uint64)
    return _flip(u[rng.permutation(len(u))])


def _window7_counts(sizes, odd=()):
    """Top-byte counts for 128 buckets (the key's top 7 bits) of the given sizes, each bucket's
    records split evenly over its two top-byte values; buckets in `odd` one record off even."""
    c = []
    for w, s in enumerate(sizes):
        hi = (s + 1) // 2 + (1 if w in odd else 0)
        c += [hi, s - hi]
    return c


class Case:
    def __init__(self, maps, R, expect, reads=None, aggs=()):
        self.maps, self.R, self.rb = maps, R, maps[0].shape[1]
        self.reads = reads or [(0, R)]
        self.expect = expect if isinstance(expect, list) else [expect] * len(self.reads)
        self.aggs = aggs


def _plan(path, lo=-1, kbits=0, window_passes=0, digit_passes=0, segmented=0, use_p=0):
    return dict(zip(NAMES, (path, lo, kbits, window_passes, digit_passes, segmented, use_p)))


# ---------------------------------------------------------------- the cases -------------
def _tiny(n):
    """n <= 256 records with distinct top bytes: maxbin = 1."""
    rng = np.random.default_rng(n)
    counts = np.zeros(256, np.int64)
    counts[rng.choice(256, n, replace=False)] = 1
    return [_rec16(_top_byte_keys(counts, rng))]


def _all_bytes_vary(n):
    """Keys whose every byte differs between any two of them (byte value 17 i + 1 throughout)."""
    return [_rec16((np.arange(n, dtype=np.uint64) * np.uint64(17) + np.uint64(1)) * np.uint64(0x0101010101010101))]


def _halo16(sizes, odd=()):
    rng = np.random.default_rng(len(sizes) + sizes[-1] + sizes[2] + sizes[4])
    assert sum(sizes) == 8192 and len(sizes) == 128
    return [_rec16(_top_byte_keys(_window7_counts(sizes, odd), rng))]


def _tail_keys(n, const, seed):
    """10-byte keys: bytes [0, const) fixed at one arbitrary value each, the rest random."""
    rng = np.random.default_rng(seed)
    kb = rng.integers(0, 256, (n, 10), dtype=np.uint8)
    kb[:, :const] = rng.integers(0, 256, const, dtype=np.uint8)[None, :]
    return kb


def _ties8(pool, seed, n=60_000):
    """First 8 key bytes drawn from `pool` random values (each recurs n / pool times on
    average), bytes 8-9 random."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (pool, 8), dtype=np.uint8)
    kb = rng.integers(0, 256, (n, 10), dtype=np.uint8)
    kb[:, :8] = p[rng.integers(0, pool, n)]
    return kb


def _halo100(sizes):
    """n = 2048 wide records, the buckets (top 5 bits of key byte 0) of the given sizes, each
    spread evenly over its 8 byte-0 values (at most 64 records per value)."""
    rng = np.random.default_rng(sizes[1])
    assert sum(sizes) == 2048 and len(sizes) == 32
    b0 = np.concatenate([np.repeat(np.arange(8) + 8 * w, _spread(s, 8)) for w, s in enumerate(sizes)])
    kb = rng.integers(0, 256, (2048, 10), dtype=np.uint8)
    kb[:, 0] = b0
    return [_rec100(kb[rng.permutation(2048)])]


def _uniform24(n, seed):
    return [_rec16(np.random.default_rng(seed).integers(0, 1 << 24, size=n))]


def _one_partition():
    """Two maps of 40 000 records sharing their keys (every key twice: real groups)."""
    rng = np.random.default_rng(1600)
    k = rng.integers(-(1 << 63), (1 << 63) - 1, size=40_000, dtype=np.int64)
    return [_rec16(k), _rec16(k[rng.permutation(len(k))], base=1 << 32)]


W_TIES8_FIT = (6500, 0)    # pool size, seed: chosen with the CPU model so that no bucket outgrows the halo
W_TIES8_OVER = (600, 1)    # ~100 records per first-8-bytes value: two in one bucket outgrow it

CASES = {
    # ---- 16 B, R = 1, one map
    # n <= 64: no window at all, the whole array is one bucket (kshift 64, wmask 0)
    "tiny16": lambda: Case(_tiny(16), 1, _plan(1, lo=64, kbits=0)),
    "tiny64": lambda: Case(_tiny(64), 1, _plan(1, lo=64, kbits=0)),
    "tiny65": lambda: Case(_tiny(65), 1, _plan(1, lo=63, kbits=1, window_passes=1)),
    # maxbin * 16 > n for every n < 16: digit passes, all eight bytes vary
    "tiny_skew2": lambda: Case(_all_bytes_vary(2), 1, _plan(0, digit_passes=8)),
    "tiny_skew15": lambda: Case(_all_bytes_vary(15), 1, _plan(0, digit_passes=8)),
    "tiny_one": lambda: Case(_all_bytes_vary(1), 1, _plan(0)),
    # top = 24: the unsegmented chunk loop below the key's top, one chunk and two (10 + 3 bits)
    "mid24": lambda: Case(_uniform24(40_000, 24), 1, _plan(1, lo=14, kbits=10, window_passes=1)),
    "mid24_two": lambda: Case(_uniform24(300_000, 25), 1, _plan(1, lo=11, kbits=13, window_passes=2)),
    # the window capped by top reaches bit 0 (kl_sh == 0: one sub-bin, order by position alone);
    # 256 buckets of exactly 128 equal keys: the max_avg boundary
    "cap_bit0": lambda: Case([_rec16((np.arange(32768) % 256)[np.random.default_rng(8).permutation(32768)])], 1,
                             _plan(1, lo=0, kbits=8, window_passes=1), aggs=("group", "sum")),
    "cap_over": lambda: Case([_rec16((np.arange(33024) % 256)[np.random.default_rng(9).permutation(33024)])], 1,
                             _plan(0, digit_passes=1)),
    "cap_shift8": lambda: Case([_rec16(((np.arange(16384) % 256) << 8)[np.random.default_rng(10).permutation(16384)])],
                               1, _plan(1, lo=8, kbits=8, window_passes=1)),
    # bytes 3..7 take two values each (0x00 / 0xFF, the top one sign-flipped): skewed, 8 digit passes
    "neg_small": lambda: Case([_rec16(np.random.default_rng(11).integers(-(1 << 23), 1 << 23, size=40_000))], 1,
                              _plan(0, digit_passes=8), aggs=("group", "sum")),
    # the halo boundary: a bucket starting on a tile's last slot fits iff its length <= HALO
    # (offset + length <= TILE + HALO - 1 = 2302); maxbin = 512 = n / 16, the skew rule at equality
    "halo_fit": lambda: Case(_halo16([1023, 1024, 255] + _spread(8192 - 2302, 125)), 1,
                             _plan(1, lo=57, kbits=7, window_passes=1)),
    "halo_over": lambda: Case(_halo16([1023, 1024, 256] + _spread(8192 - 2303, 125)), 1,
                              _plan(2, lo=57, kbits=7, window_passes=1, digit_passes=8)),
    "halo_tile1_fit": lambda: Case(_halo16([1024, 1024, 1024, 1023, 255] + _spread(8192 - 4350, 123)), 1,
                                   _plan(1, lo=57, kbits=7, window_passes=1)),
    "halo_tile1_over": lambda: Case(_halo16([1024, 1024, 1024, 1023, 256] + _spread(8192 - 4351, 123)), 1,
                                    _plan(2, lo=57, kbits=7, window_passes=1, digit_passes=8)),
    # the last bucket (1024 records, longer than the halo) is closed by the array's end (L1 == n)
    "halo_array_end": lambda: Case(_halo16(_spread(7168, 127) + [1024]), 1, _plan(1, lo=57, kbits=7, window_passes=1)),
    # halo_fit with one top-byte value at 513: maxbin * 16 > n
    "skew_over": lambda: Case(_halo16([1023, 1024, 255] + _spread(8192 - 2302, 125), odd=(1,)), 1,
                              _plan(0, digit_passes=8)),
    # ---- 16 B, R > 1
    # n <= 64 R: one pass by the partitioner, then a bucket sort whose buckets are the partitions
    "tiny_parts": lambda: Case([_rec16(np.random.default_rng(12).integers(-(1 << 63), (1 << 63) - 1, size=500,
                                                                            dtype=np.int64))], 16,
                               _plan(1, lo=64, kbits=0, window_passes=1, use_p=1), aggs=("group", "sum")),
    # a reduce task's read of one partition: no pass by the partitioner, keys of one hash residue
    "one_partition": lambda: Case(_one_partition(), 16, _plan(1, lo=57, kbits=7, window_passes=1),
                                  reads=[(0, 1), (3, 4), (15, 16)], aggs=("group", "sum")),
    # ---- 100 B, R = 1
    # bytes 0..6 constant: top 8, the window is key byte 7 and every bucket's order is bytes 8-9
    "w_tail3": lambda: Case([_rec100(_tail_keys(10_000, 7, 13))], 1, _plan(1, lo=0, kbits=8, window_passes=1)),
    # bytes 0..7 constant: nothing varies inside the 64-bit window; two digit passes (bytes 9, 8)
    "w_tail2": lambda: Case([_rec100(_tail_keys(10_000, 8, 14))], 1, _plan(0, digit_passes=2)),
    "w_prefix3": lambda: Case([_rec100(_tail_keys(30_000, 3, 15))], 1, _plan(1, lo=31, kbits=9, window_passes=1)),
    # every first-8-bytes value recurs ~10 times: the rank inside a bucket is decided by klo
    "w_ties8": lambda: Case([_rec100(_ties8(*W_TIES8_FIT))], 1, _plan(1, lo=54, kbits=10, window_passes=1)),
    "w_ties8_over": lambda: Case([_rec100(_ties8(*W_TIES8_OVER))], 1,
                                 _plan(2, lo=54, kbits=10, window_passes=1, digit_passes=10)),
    # a bucket starting on the tile's last slot: 511 + 127 = 638 = TILE + HALO - 1 fits, 128 does not
    "w_halo_fit": lambda: Case(_halo100([511, 127] + _spread(2048 - 638, 30)), 1,
                               _plan(1, lo=59, kbits=5, window_passes=1)),
    "w_halo_over": lambda: Case(_halo100([511, 128] + _spread(2048 - 639, 30)), 1,
                                _plan(2, lo=59, kbits=5, window_passes=1, digit_passes=10)),
    # HashPartitioner on wide records (use_p on k_bucket_sort<100>).  The hash takes the first 8
    # key bytes as a Long and R = 8 keeps bits 0-2 of byte 0 ^ byte 4: with w_tail3's keys those
    # are constant, every record lands in one partition, its 8 (P, window) buckets of ~375
    # records outgrow the halo, and the digit passes (bytes 9, 8, 7) + the partitioner finish.
    "w_hash": lambda: Case([_rec100(_tail_keys(3_000, 7, 16))], 8,
                           _plan(2, lo=5, kbits=3, window_passes=2, digit_passes=3, use_p=1)),
    # the same with byte 4 random too: all 8 partitions, 64 buckets of ~47, sorted on chip
    "w_hash_spread": lambda: Case([_rec100(_spread_keys())], 8, _plan(1, lo=29, kbits=3, window_passes=2, use_p=1)),
}


def _spread_keys():
    kb = _tail_keys(3_000, 7, 17)
    kb[:, 4] = np.random.default_rng(18).integers(0, 256, len(kb), dtype=np.uint8)
    return kb


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---------------------------------------------------------------- numpy reference -------
def np_order(recs):
    """Stable order by key: signed Longs, or the 10 key bytes unsigned, byte 0 most significant."""
    if recs.shape[1] == 16:
        return np.argsort(recs[:, :8].copy().view("<i8").reshape(-1), kind="stable")
    return np.lexsort(tuple(recs[:, j] for j in range(9, -1, -1)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per read of the case: (its canonical sequences, one per partition; their stable sorts,
    back to back).  Partition membership from the oracle's map side."""
    import oracle

    oracle.build()
    c = case(name)
    outs = [oracle.map_write(m, c.R) for m in c.maps]
    seqs = oracle.canonical_reducer_sequences(outs, c.R, c.rb)
    res = []
    for r0, r1 in c.reads:
        want = np.concatenate([s[np_order(s)] for s in seqs[r0:r1]])
        want.setflags(write=False)
        res.append((seqs[r0:r1], want))
    return res


def np_grouped(seqs, agg):
    keys, starts, vals, base = [], [], [], 0
    for s in seqs:
        if not len(s):
            continue
        srt = s[np_order(s)]
        k, v = srt[:, :8].copy().view("<i8").reshape(-1), srt[:, 8:].copy().view("<i8").reshape(-1)
        st = np.nonzero(np.concatenate([[True], k[1:] != k[:-1]]))[0]
        keys.append(k[st])
        starts.append(st + base)
        vals.append(v if agg == "group" else np.add.reduceat(v.view(np.uint64), st).view(np.int64))
        base += len(k)
    if agg == "group":
        return np.concatenate(keys), np.concatenate(starts), np.concatenate(vals)
    return np.concatenate(keys), np.concatenate(vals)


# ---------------------------------------------------------------- CPU: the plan, restated
def model_plan(seqs, rb, R):
    """sort_records' decisions for a fixed-codec read of the partitions `seqs` of an R-partition
    hash shuffle under flags = 0, and whether k_bucket_sort's halo holds every bucket."""
    nparts = len(seqs)
    recs = np.concatenate(seqs)
    n = len(recs)
    use_p = R > 1 and nparts != 1
    plan = _plan(0, use_p=int(use_p))
    # key bytes, most significant first; the order key's 64 bits (hi)
    cols = [recs[:, 7 - j] for j in range(8)] if rb == 16 else [recs[:, j] for j in range(10)]
    hi = np.zeros(n, np.uint64)
    for c in cols[:8]:
        hi = (hi << np.uint64(8)) | c.astype(np.uint64)
    if rb == 16:
        hi ^= np.uint64(1 << 63)
    varying = [int(np.bincount(c, minlength=256).max()) != n for c in cols]
    seg_ok = use_p and rb == 16
    rp = min(nparts, R) if use_p else 1
    kbits0 = 0
    while kbits0 < 30 and n / (rp * 2.0**kbits0) > 64.0:
        kbits0 += 1
    j = varying.index(True) if any(varying) else -1  # the most significant varying byte
    top = 64 if j < 0 else (64 - 8 * j if j < 8 else -1)
    kbits = min(kbits0, max(top, 0))
    maxbin = int(np.bincount(cols[j], minlength=256).max()) if j >= 0 else 0
    eligible = j >= 0 and top > 0 and maxbin * 16 <= n and n / (rp * 2.0**kbits) <= (128.0 if rb == 16 else 64.0)
    gave_up = False
    if eligible:
        lo = top - kbits
        seg_done = seg_ok and 1 <= kbits <= 10
        chunks = 1 if seg_done else -(-kbits // 10)
        plan.update(lo=lo, kbits=kbits, window_passes=chunks + (1 if use_p and not seg_done else 0),
                    segmented=int(seg_done))
        # after the passes the records are ordered by bucket = (P << kbits) | window; a workgroup
        # owns the buckets that start in its tile and sees HALO records past it
        win = (hi >> np.uint64(lo)) & np.uint64((1 << kbits) - 1) if kbits else np.zeros(n, np.uint64)
        pid = np.concatenate([np.full(len(s), p, np.uint64) for p, s in enumerate(seqs)])
        ids = np.sort((pid << np.uint64(kbits)) | win)
        flag = np.concatenate([[True], ids[1:] != ids[:-1]])
        T, H = TILE[rb], HALO[rb]
        for t0 in range(0, n, T):
            t1 = min(n, t0 + T)
            l1 = min(n, t1 + H)
            if flag[t0:t1].any() and not flag[t1:l1].any() and l1 != n:
                gave_up = True
        if not gave_up:
            plan["path"] = 1
            return plan
        plan["path"] = 2
    plan["digit_passes"] = sum(varying)
    if seg_ok and plan["digit_passes"]:
        plan["segmented"] = 1
    return plan


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_predict_their_branch(name):
    """The plan's arithmetic restated in numpy predicts, for every case's input, exactly the
    facts the GPU test asserts from the engine."""
    c = case(name)
    for (seqs, _), want in zip(reference(name), c.expect):
        assert model_plan(seqs, c.rb, c.R) == want


def test_low_byte_cases_decide_order_below_byte_5():
    """What the cases exist for: in w_tail3 / w_ties8 thousands of neighbours of the sorted
    output tie on key bytes 0..7 and differ in bytes 8-9 (no earlier sorted-read test has one)."""
    for name in ("w_tail3", "w_ties8", "w_tail2"):
        want = reference(name)[0][1]
        tie8 = np.all(want[1:, :8] == want[:-1, :8], axis=1) & np.any(want[1:, 8:10] != want[:-1, 8:10], axis=1)
        assert tie8.sum() > 5000, (name, int(tie8.sum()))


# ---------------------------------------------------------------- GPU -------------------
_sid = [9000]


def _read_all(sgx_lib, name, flags):
    """Write the case's maps, run each of its reads sorted (and grouped, where the case says),
    compare with numpy; returns the sorted reads' plans."""
    c = case(name)
    _sid[0] += 1
    sid = _sid[0]
    plans = []
    with sgx_lib.ShuffleEngine(device=0, num_chunks=5, flags=flags) as e:
        e.register_shuffle(sid, c.R, 0, None, True, c.rb)
        for mid, recs in enumerate(c.maps):
            e.write_map(sid, mid, np.ascontiguousarray(recs), len(recs), c.rb, c.R)
        mids = list(range(len(c.maps)))
        for (r0, r1), (seqs, want) in zip(c.reads, reference(name)):
            got = e.read_sorted(sid, mids, r0, r1).reshape(-1, c.rb)
            plans.append(e.last_sort_plan())
            assert got.shape == want.shape
            if not np.array_equal(got, want):
                bad = np.nonzero(np.any(got != want, axis=1))[0]
                pytest.fail(f"{name} [{r0}, {r1}) flags {flags}: {len(bad)} sorted records differ, first at {bad[:5]}, "
                            f"plan {plans[-1]}")
            for agg in c.aggs:
                a = sgx_lib.AGG_SUM if agg == "sum" else sgx_lib.AGG_GROUP
                res = e.read_grouped(sid, mids, r0, r1, a)
                assert e.last_sort_plan() == plans[-1], "the grouped read sorts by the same plan"
                ref = np_grouped(seqs, agg)
                assert len(res) == len(ref)
                for g, w in zip(res, ref):
                    assert np.array_equal(g, w), f"{name} [{r0}, {r1}) flags {flags}: grouped ({agg}) differs"
        e.unregister_shuffle(sid)
    return plans


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_branch_and_output(sgx_lib, oracle_lib, name):
    """flags = 0: the output equals numpy's stable sort bit for bit, and the engine reports the
    branch the case was built for."""
    plans = _read_all(sgx_lib, name, 0)
    assert plans == case(name).expect


# reads of several partitions of a fixed-codec shuffle: also with the segmented passes off
MULTI_PARTITION_CASES = ("tiny_parts", "w_hash", "w_hash_spread")


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", [(n, f) for n in sorted(CASES) for f in (64, 128)] +
                         [(n, 1024) for n in MULTI_PARTITION_CASES])
def test_output_under_other_plans(sgx_lib, oracle_lib, name, flags):
    """The same inputs with the bucket path off (64: digit passes only), on the ballot-ranked
    kernels (128) and, for multi-partition reads, with the segmented passes off (1024)."""
    plans = _read_all(sgx_lib, name, flags)
    if flags == 64:
        assert all(p["path"] == 0 and p["lo"] == -1 for p in plans)
    if flags == 1024:
        assert all(p["segmented"] == 0 for p in plans)
