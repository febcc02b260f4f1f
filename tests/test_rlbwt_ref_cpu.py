"""CPU suite: tests/rlbwt_ref.py build_rows_rl -- the run-length restatement that tests/test_build_big_text_gpu.py holds the GPU builder
to on texts of 2^31 characters and more -- is itself held to oracle/build_index.py build_rows, byte for byte on whole images, on every
input of tests/test_build_rlbwt_gpu.py that build_rows can take and on 240 random small tables.  Then, from build_rows_rl alone, what
the big tables must contain for a position computed in 32 bits to show in the image."""
import numpy as np
import pytest

from oracle import build_index as B
import odd_texts
import rlbwt_ref as R
import test_build_rlbwt_gpu as G

MODES = G.MODES


def same_as_build_rows(bwt, thr, mode):
    bwt, thr = np.asarray(bwt, np.uint8), np.asarray(thr, np.int64)
    heads, lens = R.rle(bwt)
    f = R.build_rows_rl(heads, lens, thr, mode)
    assert G.same(B.serialize(f), B.serialize(B.build_rows(bwt, thr, mode)))
    return f


@pytest.mark.parametrize("separators", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_golden_text(mode, separators):
    bwt, thr = G.golden_table(separators)
    f = same_as_build_rows(bwt, thr, mode)
    assert len(B.serialize(f)) == G.KAT[(mode, separators)]


@pytest.mark.parametrize("kind,separators,mode", [(k, False, m) for k in odd_texts.KINDS for m in MODES] +
                         [(k, True, m) for k in ("poly", "tandem") for m in (6, 8, 7)])
def test_odd_texts(kind, separators, mode):
    bwt, thr, _ = odd_texts.table(kind, separators)
    heads, lens = R.rle(bwt)
    assert G.same(B.serialize(R.build_rows_rl(heads, lens, thr, mode)), odd_texts.fields(kind, separators, mode)[1])


@pytest.mark.parametrize("mode", MODES)
def test_hand_made_thresholds(mode):
    """The table of test_build_rlbwt_gpu.py::test_hand_made_thresholds."""
    runs = [("A", 5), ("C", 3000), ("G", 7), ("A", 5000), ("T", 2), (0, 1), ("C", 40), ("G", 4100), ("A", 1), ("T", 600)]
    st = G.starts_of(runs)
    n = int(sum(k for _, k in runs))
    thr = np.zeros(len(runs), np.int64)
    thr[1] = st[3]
    thr[2] = thr[4] = st[3] + 1500
    thr[3] = st[1] + B.MAX_RUN[mode]
    thr[6] = st[7] + 4099
    thr[7] = n
    thr[8] = st[5]
    thr[9] = st[7] + 1
    same_as_build_rows(G.expand(runs), thr, mode)


@pytest.mark.parametrize("place", sorted(G.TERMINATOR_PLACES))
@pytest.mark.parametrize("mode", MODES)
def test_terminator_places(mode, place):
    runs = G.TERMINATOR_PLACES[place]
    st = G.starts_of(runs)
    rng = np.random.default_rng(len(place))
    for thr in (np.zeros(len(runs), np.int64), st[rng.integers(0, len(runs), len(runs))], rng.integers(0, int(st[-1]) + 1, len(runs))):
        same_as_build_rows(G.expand(runs), thr, mode)


@pytest.mark.parametrize("mode", (7, 5))
@pytest.mark.parametrize("r", (39, 40, 41, 20 * 300 - 1, 20 * 300, 20 * 300 + 1))
def test_rows_around_a_tally_checkpoint(mode, r):
    runs = G.singles(r // 2) + [(0, 1)] + G.singles(r - r // 2 - 1, b"CAGT")
    f = same_as_build_rows(G.expand(runs), np.zeros(len(runs), np.int64), mode)
    assert f["r"] == r and f["tally_ids"].shape[1] == r // 20 + 2


ALPHABETS = (b"A", b"CT", b"ACG", b"ACGT", b"%ACGT")


def random_table(rng, letters):
    """A small table over exactly `letters`: the terminator anywhere (first and last included), most runs short, some longer than every
    MAX_RUN_LENGTH, thresholds anywhere in [0, n] -- some of them equal, some on run starts, some n."""
    if len(letters) == 1:
        heads = [[0, letters[0]], [letters[0], 0], [letters[0], 0, letters[0]]][int(rng.integers(0, 3))]
    else:
        k = int(rng.integers(len(letters), 40))
        heads = list(rng.permutation(list(letters)))                 # every letter at least once
        while len(heads) < k:
            c = letters[int(rng.integers(0, len(letters)))]
            if c != heads[-1]:
                heads.append(c)
        heads.insert([0, len(heads), int(rng.integers(0, len(heads) + 1))][int(rng.integers(0, 3))], 0)
        for i in range(len(heads) - 1, 0, -1):                       # the terminator may have left two equal neighbours: no such pair
            if heads[i] == heads[i - 1]:
                del heads[i]
    heads = np.array(heads, np.uint8)
    lens = rng.integers(1, 6, heads.size)
    long = rng.random(heads.size) < 0.15
    lens[long] = rng.integers(400, 9000, int(long.sum()))
    lens[heads == 0] = 1
    n = int(lens.sum())
    thr = rng.integers(0, n + 1, heads.size)
    st = np.cumsum(lens) - lens
    pick = rng.random(heads.size)
    thr[pick < 0.15] = st[rng.integers(0, heads.size, int((pick < 0.15).sum()))]
    thr[pick > 0.9] = [0, n, int(thr[0])][int(rng.integers(0, 3))]
    return heads, lens, thr


@pytest.mark.parametrize("letters", ALPHABETS)
def test_random_small_tables(letters):
    """48 tables per alphabet, 240 in all, each in one of the six types in turn."""
    rng = np.random.default_rng(len(letters) * 7919)
    for k in range(48):
        heads, lens, thr = random_table(rng, letters)
        assert (heads[1:] != heads[:-1]).all() and set(heads.tolist()) == set(letters) | {0}
        mode = MODES[k % 6]
        f = R.build_rows_rl(heads, lens, thr, mode)
        want = B.build_rows(np.repeat(heads, lens), thr, mode)
        assert G.same(B.serialize(f), B.serialize(want)), (letters, k, mode)
        assert f["sep"] == (letters[0] == 37)


# ---- what the big tables must contain (asserts on the reference's fields; tests/test_build_big_text_gpu.py builds these tables)

BIG = [("2^31", False), ("2^32", False), ("2^32", True), ("2^33", False)]


@pytest.mark.parametrize("name,separators", BIG)
def test_big_table_conditions(name, separators):
    n = R.BIG_N[name]
    heads, lens, thr, edge = R.big_table(n, separators)
    assert int(lens.sum()) == n and edge == {"2^31": 1 << 31, "2^32": 1 << 32, "2^33": 1 << 32}[name]
    assert len(set(heads.tolist())) == (6 if separators else 5)
    # thresholds either side of the edge and of n, among the runs' thresholds
    for v in (edge - 1, edge, edge + 1, n - 1, n):
        assert (thr == v).any(), v
    if name == "2^33":
        assert int((lens >= (1 << 32)).sum()) == 1
    for mode in (6, 3):
        f, img = R.big_fields(n, separators, mode)
        assert f["n"] == n and int(np.frombuffer(img, "<u8", 1, 16)[0]) == n
        assert f["r"] > n // B.MAX_RUN[mode]
        # ids and offsets that depend on the high bits: LF targets past the edge, in rows shorter than MAX_RUN_LENGTH (a target
        # inside a full row of the giant run would get the same offset from many a wrong position)
        far = (f["lf"] >= edge) & (f["lens"][f["pp_id"]] < B.MAX_RUN[mode])
        assert int(far.sum()) >= 1000, int(far.sum())
        assert (f["all_p"][f["pp_id"][far]] >= edge).all()
        if mode == 6:
            # rows that exist only because a threshold past the edge split a run there
            by_thr = (f["all_p"] >= edge) & np.isin(f["all_p"], thr) & ~np.isin(f["all_p"], f["run_start"])
            assert int(by_thr.sum()) >= 1000, int(by_thr.sum())
            if separators:
                assert len(f["sep_thr"]) >= 2 and len(f["sep_map"]) == len(f["sep_thr"])


@pytest.mark.parametrize("name,separators,mode", [("2^31", False, 8), ("2^31", False, 2), ("2^32", False, 8), ("2^32", False, 2), ("2^32", True, 8)])
def test_big_tables_keep_the_default_block_size(name, separators, mode):
    """oracle/build_index.py compute_blocked_ids is wrong once the block size must halve (test_build_rlbwt_gpu.py::
    test_block_size_halves): the big tables must not need that, in the blocked types they are built in."""
    f, _ = R.big_fields(R.BIG_N[name], separators, mode)
    assert f["block_size"] == B.BLOCK_SIZE[mode] and f["id_blocks"].shape[1] == (f["r"] + f["block_size"] - 1) // f["block_size"]
