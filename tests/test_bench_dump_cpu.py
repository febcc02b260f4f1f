"""CPU suite: bench.py --dump-outputs -- what one step computed, written as float32 / float64 .npy files, sampled by whole reads
in a fixed seeded order when the batch is larger than the dump's caps."""
import numpy as np
import torch

import bench


def _dump(tmp_path, offs, per_base, per_read):
    bench.dump_outputs(str(tmp_path), offs, per_base, per_read)
    return {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}


def test_small_batch_is_written_whole(tmp_path):
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 300, size=1000).astype(np.uint64)
    offs = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    pml = torch.from_numpy(rng.integers(0, 1 << 16, size=int(offs[-1])).astype(np.uint16).view(np.int16))
    count = torch.from_numpy(rng.integers(0, 1 << 40, size=1000).astype(np.int64))
    err = torch.from_numpy(rng.integers(0, 2, size=1000).astype(np.uint8))
    got = _dump(tmp_path, offs, {"pml": pml}, {"count": count, "errors": err})
    assert set(got) == {"pml", "count", "errors", "read_ids"}
    assert got["pml"].dtype == np.float32 and got["errors"].dtype == np.float32
    assert got["count"].dtype == np.float64 and got["read_ids"].dtype == np.float64
    assert np.array_equal(got["pml"], pml.numpy().view(np.uint16))             # u16 PMLs, not their int16 bit pattern
    assert np.array_equal(got["count"], count.numpy()) and np.array_equal(got["errors"], err.numpy())
    assert np.array_equal(got["read_ids"], np.arange(1000))


def test_large_batch_is_a_fixed_sample_of_whole_reads(tmp_path):
    n, L = 200_000, 150                                             # 30 M bases: beyond DUMP_MAX_BASES
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    vec = torch.from_numpy((np.arange(n * L, dtype=np.int64) % 65521).astype(np.uint16).view(np.int16))
    per_read = torch.from_numpy(np.arange(n, dtype=np.int64) * 3)
    a = _dump(tmp_path / "a", offs, {"pml": vec}, {"matched": per_read})
    b = _dump(tmp_path / "b", offs, {"pml": vec}, {"matched": per_read})
    for k in a:
        assert np.array_equal(a[k], b[k]), k                          # the same sample every time
    ids = a["read_ids"].astype(np.int64)
    assert 0 < ids.size * L <= bench.DUMP_MAX_BASES and ids.size > bench.DUMP_MAX_BASES // L - 1
    assert np.all(np.diff(ids) > 0)                                  # sorted, no read twice
    pos = (ids[:, None] * L + np.arange(L)).ravel()                  # every sampled read whole, in read order
    assert np.array_equal(a["pml"], pos % 65521)
    assert np.array_equal(a["matched"], ids * 3)
    total = sum((tmp_path / "a" / (k + ".npy")).stat().st_size for k in a)
    assert total <= 64 << 20
