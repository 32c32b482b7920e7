"""reduceByKey(min) / reduceByKey(max) / per-key counts on the GPU (SGX_AGG_MIN / _MAX / _COUNT),
reduce side and map-side combine, against numpy: the oracle has no min / max / count.

* reduction: a stable argsort of each reducer's canonical sequence by key, then
  np.minimum.reduceat / np.maximum.reduceat over the group starts, or their np.diff (count);
* combiners: the same reduction inside each partition slice of oracle.map_write(recs, R), keys
  ascending within the partition (the canonical order SUM's combiners already have).

Reading a combined shuffle is combineCombinersByKey: min of minima, max of maxima, and the SUM
of the maps' counts (Aggregator.mergeCombiners, not mergeValue) -- so every combined read is
compared with the reduction of the RAW records.
"""
import ctypes

import numpy as np
import pytest

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
GI, WAVE, T, WINDOW = 16, 64 * 16, 4096, 64  # k_group_fused: run, wave, tile (records); look-back window (tiles)
OPS = ("min", "max", "count")


def agg_of(sgx_lib, op):
    return {"min": sgx_lib.AGG_MIN, "max": sgx_lib.AGG_MAX, "count": sgx_lib.AGG_COUNT, "sum": sgx_lib.AGG_SUM,
            "group": sgx_lib.AGG_GROUP}[op]


def records(keys, vals):
    recs = np.empty((len(keys), 16), np.uint8)
    recs[:, :8] = np.ascontiguousarray(keys, dtype=np.int64).view(np.uint8).reshape(-1, 8)
    recs[:, 8:] = np.ascontiguousarray(vals, dtype=np.int64).view(np.uint8).reshape(-1, 8)
    return recs


def kv(recs):
    a = np.ascontiguousarray(recs).view("<i8").reshape(-1, 2)
    return a[:, 0], a[:, 1]


def reduce_runs(v, starts, n, op):
    if op == "min":
        return np.minimum.reduceat(v, starts)
    if op == "max":
        return np.maximum.reduceat(v, starts)
    return np.diff(np.append(starts, n)).astype(np.int64)


def expect_reduced(seqs, op):
    """(keys, values) of the reducers' canonical sequences, reducer-major, keys ascending."""
    ks, vs = [np.empty(0, np.int64)], [np.empty(0, np.int64)]
    for s in seqs:
        if not len(s):
            continue
        k, v = kv(s)
        order = np.argsort(k, kind="stable")
        k, v = k[order], v[order]
        starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
        ks.append(k[starts])
        vs.append(reduce_runs(v, starts, len(k), op))
    return np.concatenate(ks), np.concatenate(vs)


def expect_combiners(oracle_lib, recs, R, op):
    """One map's combined output: ({key, combiner} records partition-contiguous, counts[R])."""
    out, counts = oracle_lib.map_write(recs, R)
    k, v = kv(out)
    pid = np.repeat(np.arange(R), counts)
    order = np.lexsort((k, pid))  # stable: by partition, then key
    k, v, pid = k[order], v[order], pid[order]
    starts = np.flatnonzero(np.r_[True, (k[1:] != k[:-1]) | (pid[1:] != pid[:-1])]) if len(k) else np.empty(0, np.int64)
    if not len(k):
        return np.empty((0, 16), np.uint8), np.zeros(R, np.int64)
    return records(k[starts], reduce_runs(v, starts, len(k), op)), np.bincount(pid[starts], minlength=R).astype(np.int64)


def raw_sequences(oracle_lib, maps, R):
    return oracle_lib.canonical_reducer_sequences([oracle_lib.map_write(m, R) for m in maps], R, 16)


# ---------------------------------------------------------------------------------------
# 1. tile shapes x operator x value set
# ---------------------------------------------------------------------------------------
SHAPES = {
    # every boundary of the scan: run, wave, tile, and one group longer than a look-back window
    "boundaries": [1, 15, 16, 17, WAVE - 1, WAVE, WAVE + 1, T - 1, T, T + 1, 3 * T + 17, (WINDOW + 2) * T + 5, 1],
    "unique": [1] * (2 * T + 1),
    "single": [1],
}
VALUE_SETS = ("positive", "negative", "mixed", "extremes")


def shaped_maps(shape, values):
    """Two maps (R = 1) whose keys, sorted, form groups of the given sizes."""
    sizes = np.array(SHAPES[shape], np.int64)
    n = int(sizes.sum())
    rng = np.random.default_rng(n * 7 + VALUE_SETS.index(values))
    gkeys = np.sort(rng.permutation(1 << 20)[:len(sizes)].astype(np.int64) - (1 << 19)) * 0x3B9ACA07  # distinct, both signs
    keys = np.repeat(gkeys, sizes)[rng.permutation(n)]
    if values == "positive":    # a zero identity would win every minimum
        vals = rng.integers(1 << 40, 1 << 62, size=n, dtype=np.int64)
    elif values == "negative":  # ... and every maximum
        vals = rng.integers(-(1 << 62), -(1 << 40), size=n, dtype=np.int64)
    elif values == "mixed":     # an unsigned compare orders negatives above positives
        vals = rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
    else:
        # the identities themselves as values: in the first, a middle and the last record (sorted,
        # canonical order) of the two largest groups, small values around them
        vals = rng.integers(-1000, 1000, size=n, dtype=np.int64)
        order = np.argsort(keys, kind="stable")  # R = 1: the canonical sequence is map 0, then map 1
        off = np.concatenate([[0], np.cumsum(sizes)])
        big = np.argsort(sizes, kind="stable")[::-1][:2]
        for g, (edge, mid) in zip(big, ((I64_MIN, I64_MAX), (I64_MAX, I64_MIN))):
            a, b = int(off[g]), int(off[g + 1])
            vals[order[a]] = edge
            vals[order[(a + b) // 2]] = mid
            vals[order[b - 1]] = edge
    recs = records(keys, vals)
    cut = n // 3
    return [recs[:cut], recs[cut:]]


@pytest.mark.gpu
@pytest.mark.parametrize("values", VALUE_SETS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_shapes(sgx_lib, oracle_lib, shape, values):
    maps = shaped_maps(shape, values)
    seqs = raw_sequences(oracle_lib, maps, 1)
    n = sum(len(m) for m in maps)
    with sgx_lib.ShuffleEngine(device=0) as e:
        e.register_shuffle(1, 1)
        for m, recs in enumerate(maps):
            e.write_map(1, m, np.ascontiguousarray(recs), len(recs), 16, 1)
        # MIN then MAX with identical arguments: the read cache is keyed by the aggregation
        for op in OPS:
            wk, wv = expect_reduced(seqs, op)
            assert len(wk) == len(SHAPES[shape])
            keys, vals = e.read_grouped(1, [0, 1], 0, 1, agg_of(sgx_lib, op))
            assert np.array_equal(keys, wk), op
            bad = np.flatnonzero(vals != wv) if len(vals) == len(wv) else None
            assert bad is not None and not len(bad), (op, None if bad is None else
                                                      (bad[:4], vals[bad[:4]], wv[bad[:4]]))
            assert e.last_read_records() == n


# ---------------------------------------------------------------------------------------
# 2. partitioned reads
# ---------------------------------------------------------------------------------------
def skewed_maps():
    rng = np.random.default_rng(0xA66)
    zk = (rng.zipf(1.2, size=40_000) % 5000).astype(np.int64) * 0x9E3779B1 - (1 << 43)
    uk = rng.integers(-(1 << 62), 1 << 62, size=10_000, dtype=np.int64)
    zk[::7] = uk[:len(zk[::7])]  # keys the maps share
    return [records(zk, rng.integers(-(1 << 62), 1 << 62, size=len(zk), dtype=np.int64)),
            records(uk, rng.integers(-(1 << 62), 1 << 62, size=len(uk), dtype=np.int64)),
            records(zk[:1], np.array([I64_MIN], np.int64))]


def size_query(sgx_lib, e, sid, maps, r0, r1, agg):
    m = np.ascontiguousarray(maps, dtype=np.int64)
    ng, nv = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = sgx_lib.lib().sgx_read_grouped(e.handle, sid, m.ctypes.data, len(m), r0, r1, agg, None, None, None, 0, 0,
                                        sgx_lib.MEM_HOST, ctypes.byref(ng), ctypes.byref(nv))
    assert rc == 0
    return ng.value, nv.value


@pytest.mark.gpu
@pytest.mark.parametrize("R,codec", [(1, "fixed"), (200, "fixed"), (1024, "fixed"), (200, "kryo+lz4")])
def test_partitioned_reads(sgx_lib, oracle_lib, R, codec):
    maps = skewed_maps()
    seqs = raw_sequences(oracle_lib, maps, R)
    with sgx_lib.ShuffleEngine(device=0) as e:
        e.register_shuffle(1, R, serializer=sgx_lib.SER_FIXED if codec == "fixed" else sgx_lib.SER_KRYO)
        if codec == "kryo+lz4":
            e.set_compression(1, "lz4", 32768)
        for m, recs in enumerate(maps):
            e.write_map(1, m, recs, len(recs), 16, R)
        for op in OPS:
            agg = agg_of(sgx_lib, op)
            for r0, r1 in ((0, R), (1, R), (R // 2, R // 2)):
                wk, wv = expect_reduced(seqs[r0:r1], op)
                nrec = sum(len(s) for s in seqs[r0:r1])
                assert size_query(sgx_lib, e, 1, [0, 1, 2], r0, r1, agg) == (len(wk), len(wk))
                keys, vals = e.read_grouped(1, [0, 1, 2], r0, r1, agg)
                assert np.array_equal(keys, wk) and np.array_equal(vals, wv), (op, r0, r1)
                assert e.last_read_records() == nrec
                if r0 == r1:
                    assert len(keys) == 0 and len(vals) == 0


# ---------------------------------------------------------------------------------------
# 3. map-side combine
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("codec", ["fixed", "kryo+lz4"])
@pytest.mark.parametrize("R,n,distinct", [(1, 10_000, 50), (200, 100_000, 20_000), (4096, 50_000, 700)])
def test_map_side_combine(sgx_lib, oracle_lib, op, codec, R, n, distinct):
    rng = np.random.default_rng(n + R)
    pool = rng.integers(-(1 << 62), 1 << 62, size=distinct, dtype=np.int64)
    maps = [records(pool[rng.integers(0, distinct, size=n + m)],
                    rng.integers(-(1 << 63), (1 << 63) - 1, size=n + m, dtype=np.int64)) for m in range(2)]
    agg = agg_of(sgx_lib, op)

    def want_bytes(recs):
        out, counts = expect_combiners(oracle_lib, recs, R, op)
        if codec == "fixed":
            return out.reshape(-1), counts * 16
        kryo = oracle_lib.kryo_serialize(out)
        return oracle_lib.lz4_frame_partitions(kryo, oracle_lib.kryo_partition_offsets(out, counts))

    with sgx_lib.ShuffleEngine(device=0) as e:
        for sid in (1, 2):
            e.register_shuffle(sid, R, serializer=sgx_lib.SER_FIXED if codec == "fixed" else sgx_lib.SER_KRYO)
            if codec == "kryo+lz4":
                e.set_compression(sid, "lz4", 32768)
            e.set_map_side_combine(sid, agg)
        for m, recs in enumerate(maps):
            lengths = e.write_map(1, m, recs, len(recs), 16, R)
            data, lens = want_bytes(recs)
            assert np.array_equal(lengths, lens), m
            assert np.array_equal(e.map_output_bytes(1, m), data), m
        # the reader merges combiners: the result is the reduction of the raw records (for
        # count: the maps' counts summed, not the combiners counted)
        wk, wv = expect_reduced(raw_sequences(oracle_lib, maps, R), op)
        keys, vals = e.read_grouped(1, [0, 1], 0, R, agg)
        assert np.array_equal(keys, wk) and np.array_equal(vals, wv)
        assert e.last_read_records() == sum(int(c.sum()) for _, c in (expect_combiners(oracle_lib, r, R, op) for r in maps))
        # a streaming map: the same bytes as one write of the concatenation
        recs = maps[0]
        cuts = [0, len(recs) // 5, len(recs) // 5 + 1, len(recs)]
        e.map_begin(2, 0)
        for a, b in zip(cuts[:-1], cuts[1:]):
            e.map_append(2, 0, np.ascontiguousarray(recs[a:b]), b - a, 16)
        assert np.array_equal(e.map_commit(2, 0, R), e.map_lengths(1, 0, R))
        assert np.array_equal(e.map_output_bytes(2, 0), e.map_output_bytes(1, 0))


# ---------------------------------------------------------------------------------------
# 4. errors
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors(sgx_lib):
    rng = np.random.default_rng(4)
    recs = records(rng.integers(0, 9, size=100), rng.integers(-5, 5, size=100))
    with sgx_lib.ShuffleEngine(device=0) as e:
        e.register_shuffle(1, 8)
        e.set_map_side_combine(1, sgx_lib.AGG_MIN)
        e.register_shuffle(2, 8)
        for bad in (sgx_lib.AGG_GROUP, 99):
            with pytest.raises(sgx_lib.UnsupportedOperationException):
                e.set_map_side_combine(2, bad)
        e.write_map(1, 0, recs, len(recs), 16, 8)
        e.write_map(2, 0, recs, len(recs), 16, 8)
        for other in (sgx_lib.AGG_MAX, sgx_lib.AGG_SUM, sgx_lib.AGG_GROUP, sgx_lib.AGG_COUNT):
            with pytest.raises(sgx_lib.UnsupportedOperationException):
                e.read_grouped(1, [0], 0, 8, other)
        keys, vals = e.read_grouped(1, [0], 0, 8, sgx_lib.AGG_MIN)
        k, v = kv(recs)
        assert sorted(keys.tolist()) == sorted(set(k.tolist()))
        assert all(v[k == key].min() == val for key, val in zip(keys.tolist(), vals.tolist()))
        for sid in (1, 2):
            with pytest.raises(sgx_lib.IllegalStateException):
                e.set_map_side_combine(sid, sgx_lib.AGG_MAX)
        with pytest.raises(sgx_lib.IllegalArgumentException):
            e.read_grouped(2, [0], 0, 8, 99)
        # shuffle 2 was not combined: every aggregation reads it
        assert len(e.read_grouped(2, [0], 0, 8, sgx_lib.AGG_COUNT)[0]) == len(set(k.tolist()))


# ---------------------------------------------------------------------------------------
# 5. plugin mirror
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("combine", [False, True])
@pytest.mark.parametrize("op", OPS)
def test_plugin_mirror(sgx_lib, oracle_lib, op, combine):
    R = 64
    rng = np.random.default_rng(5)
    pool = rng.integers(-(1 << 62), 1 << 62, size=3000, dtype=np.int64)
    maps = [records(pool[rng.integers(0, len(pool), size=n)], rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64))
            for n in (20_000, 5_001)]
    wk, wv = expect_reduced(raw_sequences(oracle_lib, maps, R), op)
    shuffled = sum(int(expect_combiners(oracle_lib, m, R, op)[1].sum()) for m in maps) if combine else sum(map(len, maps))
    mgr = sgx_lib.UcxShuffleManager(device=0)
    try:
        dep = sgx_lib.ShuffleDependency(sgx_lib.HashPartitioner(R), 16, aggregator=sgx_lib.Aggregator(op),
                                        mapSideCombine=combine)
        h = mgr.registerShuffle(3, dep)
        for m, recs in enumerate(maps):
            mgr.getWriter(h, m).write(recs)
        rd = mgr.getReader(h, 0, R)
        keys, vals = rd.read()
        assert np.array_equal(keys, wk) and np.array_equal(vals, wv)
        assert rd.readMetrics.recordsRead == shuffled  # the shuffled records, not the groups
        rd = mgr.getReader(h, 0, R)
        assert list(rd.iterator()) == list(zip(wk.tolist(), wv.tolist()))
        assert rd.readMetrics.recordsRead == shuffled
    finally:
        mgr.stop()


# ---------------------------------------------------------------------------------------
# CPU: what stays refused
# ---------------------------------------------------------------------------------------
def test_unknown_aggregator_still_refused(sgx_lib):
    with pytest.raises(sgx_lib.IllegalArgumentException):
        sgx_lib.Aggregator("median")
    for kind in ("group", "sum") + OPS:
        assert sgx_lib.Aggregator(kind).kind == kind


def test_group_never_combines_map_side(sgx_lib):
    with pytest.raises(sgx_lib.UnsupportedOperationException):
        sgx_lib.ShuffleDependency(sgx_lib.HashPartitioner(4), 16, aggregator=sgx_lib.Aggregator("group"),
                                  mapSideCombine=True)
    with pytest.raises(sgx_lib.IllegalArgumentException):
        sgx_lib.ShuffleDependency(sgx_lib.HashPartitioner(4), 16, mapSideCombine=True)
    for kind in ("sum",) + OPS:
        dep = sgx_lib.ShuffleDependency(sgx_lib.HashPartitioner(4), 16, aggregator=sgx_lib.Aggregator(kind),
                                        mapSideCombine=True)
        assert dep.mapSideCombine
