"""Text positions of count and MEM hits (movi_locate_matches_device) on a device-resident batch: items/s and positions/s at
max_occ 1, 10 and 100, and where the time goes -- interval search + scan, expansion, locate walk -- from HIP events.

  python tools/locate_matches_bench.py [--repeats N] [--sample-rate R] [--reads N]

Workload: bench.py's c2 pangenome (64 genomes, 14 M rows) with the first --reads of its 1 M x 150 bp reads (default: all); interval
table K = 12; sampled suffix array of --sample-rate (default 100, built here with movi_ssa_build).  Two item sources, as the command
line builds them: COUNT -- one item (i, len - matched, len) per read with matched > 0 of movi_count_host --, and MEM -- one item per
MEM of movi_mem_host at L = 25.  Every figure: one warm-up call, then the median of --repeats calls, each between two HIP events.
The split comes from the "locate_matches_stages" option: the call stopped after the scan (1), after the expansion (2), and whole (3);
the differences are the expansion's and the walk's time.  One JSON line per (item source, max_occ)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(torch, fn, repeats):
    """Median of `repeats` calls in ms, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample-rate", type=int, default=100)
    ap.add_argument("--reads", type=int, default=0)
    args = ap.parse_args()
    import torch
    import bench
    import movi_amd
    dev = torch.device("cuda", 0)
    wl = dict(bench.WORKLOADS["c2"])
    idx_dir, reads_file = bench.ensure_pangenome(wl, 1, 0, lambda: None)
    n, rl = wl["reads"], wl["read_len"]
    if args.reads:
        n = min(n, args.reads)
    bases = np.fromfile(reads_file, np.uint8, count=n * rl)
    offs = (np.arange(n + 1, dtype=np.uint64) * np.uint64(rl))
    ix = movi_amd.MoveIndex.load(idx_dir)
    ix.set_option("ftab_k", 12)
    ix.build_ssa(args.sample_rate)
    ix.prepare(ix.PREPARE_COUNT | ix.PREPARE_SA)
    # the item sources
    matched, _, _ = ix.query_count_packed(bases, offs)
    has = np.flatnonzero(matched > 0)
    count_items = np.zeros(has.size, ix.MATCH_DTYPE)
    count_items["read"], count_items["start"], count_items["end"] = has, rl - matched[has], rl
    nm, mems, _ = ix.query_mems_packed(bases, offs, 25)
    mem_items = np.zeros(mems.size, ix.MATCH_DTYPE)
    mem_items["read"] = np.repeat(np.arange(n, dtype=np.uint32), nm)
    mem_items["start"], mem_items["end"] = mems["start"], mems["end"]
    db, do = torch.from_numpy(bases).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev)
    for source, items in (("count", count_items), ("mem", mem_items)):
        ni = int(items.size)
        if ni == 0:
            continue
        di = torch.from_numpy(np.frombuffer(items.tobytes(), np.uint8).copy()).to(dev)
        docc = torch.empty(ni, dtype=torch.int64, device=dev)
        dfirst = torch.empty(ni + 1, dtype=torch.int64, device=dev)
        wb = ix.locate_matches_work_bytes(ni)
        dwork = torch.empty(wb, dtype=torch.uint8, device=dev)
        mean_len = float((items["end"].astype(np.int64) - items["start"]).mean())
        for max_occ in (1, 10, 100):
            cap = ni * max_occ
            dpos = torch.empty(cap, dtype=torch.int64, device=dev)
            call = lambda: ix.locate_matches_device(db.data_ptr(), do.data_ptr(), n, di.data_ptr(), ni, max_occ, docc.data_ptr(),
                                                    dfirst.data_ptr(), dpos.data_ptr(), cap, dwork.data_ptr(), wb)
            t = {}
            for stage in (1, 2, 3):
                ix.set_option("locate_matches_stages", stage)
                t[stage] = timed(torch, call, args.repeats)
                if stage == 1:
                    st1 = ix.last_stats()
            st = ix.last_stats()                                  # the whole call: search steps + LF steps of the walks
            kernel = ix.last_launch()["kernel"]
            total = int(dfirst[-1].item())
            occ = docc.cpu().numpy().view(np.uint64)
            pos = dpos[:total].cpu().numpy().view(np.uint64)
            walk_steps = st.lane_steps - st1.lane_steps
            print(json.dumps({
                "workload": "c2", "source": source, "reads": n, "read_len": rl, "rows": ix.desc.r, "text": int(ix.desc.length),
                "sample_rate": args.sample_rate, "ftab_k": 12, "items": ni, "mean_item_len": round(mean_len, 1), "max_occ": max_occ,
                "positions": total, "items_with_more": int((occ > max_occ).sum()), "max_occ_seen": int(occ.max()),
                "pos_none": int((pos == np.uint64(ix.POS_NONE)).sum()), "errors": int(st.errors),
                "total_ms": round(t[3], 3), "search_scan_ms": round(t[1], 3), "expand_ms": round(t[2] - t[1], 3),
                "walk_ms": round(t[3] - t[2], 3), "mitems_s": round(ni / t[3] / 1e3, 2), "mpositions_s": round(total / t[3] / 1e3, 2),
                "search_steps_per_item": round(st1.lane_steps / ni, 2), "lf_steps_per_position": round(walk_steps / max(total, 1), 2),
                "search_occupancy": round(st1.lane_steps / (64.0 * st1.wave_steps), 3) if st1.wave_steps else None,
                "last_kernel": kernel}), flush=True)
            del dpos
        del di, docc, dfirst, dwork
    ix.set_option("locate_matches_stages", 3)
    ix.close()


if __name__ == "__main__":
    main()
