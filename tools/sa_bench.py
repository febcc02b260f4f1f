"""Locate next to the PML walk on the same device-resident batch (movi_ssa_build, movi_locate_device, movi_sa_entries_device vs
movi_pml_device, HIP events).

  python tools/sa_bench.py [--steps N] [--only c2|c3] [--rate R] [--reads N] [--out profiles/sa_bench.txt]

Workloads: bench.py's c2 pangenome (64 genomes, 14 M rows) with 150 bp reads, and its c3 batch of 10 kbp reads (8 % substitutions);
--reads caps the reads taken (default 100 k / 2 k: at rate 100 a base costs about a hundred gathers).  One JSON line per workload,
appended to --out as well:
  build_sa_s            movi_ssa_build, seconds (c2: the `build-SA` figure)
  sa_entries_gbases     movi_sa_entries_device, Gbases/s of read bases
  locate_steps_per_s    LF steps of the locate kernel per second (movi_last_stats lane_steps over the call's time)
  locate_lines_per_s    the same as 128-byte lines: one 16-byte gather per step + the fast-forwards' rows
  pml_lines_per_s       the PML walk's line rate on the same table, from profiles/r06_bench_default.json: roofline.traffic / 128 over
                        the kernel's time (the locate walk's ceiling is the same random-gather rate)
  walk_mean             LF steps per position, against `rate`; walk_max_of_256: the longest of 256 single walks spread over the table
  occupancy             lane_steps / (64 x wave_steps) of the strided-item loop"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(torch, fn, steps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def pml_line_rate(wl_name):
    """128-byte lines per second of the PML walk on this workload, from profiles/r06_bench_default.json: the bytes the walk kernel
    moved per step (roofline.traffic, from its counter passes) over 128 and over the kernel's time.  c2 is that file's main leg, c3 its
    long_reads leg.  A file without these keys is an error: the figure is what the locate rate is held against."""
    d = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_default.json")))
    leg, name = (d, d["config"]["workload"]) if wl_name == "c2" else (d["long_reads"], d["long_reads"]["workload"])
    if name != wl_name:
        raise KeyError("profiles/r06_bench_default.json holds %r where %r was expected" % (name, wl_name))
    roof = leg["roofline"]
    return roof["traffic"] / 128.0 / (roof["kernel_ms_avg"] * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--rate", type=int, default=100)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_bench.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import movi_amd
    dev = torch.device("cuda", 0)
    for wl_name in ("c2", "c3"):
        if args.only and args.only != wl_name:
            continue
        pml_rate = pml_line_rate(wl_name)                  # (first: a profile without the figure stops the run before any work)
        wl = dict(bench.WORKLOADS[wl_name])
        idx_dir, reads_file = bench.ensure_pangenome(wl, 1, 0, lambda: None)
        rl = wl["read_len"]
        n = min(wl["reads"], args.reads or (100000 if rl < 1024 else 2000))
        nb = n * rl
        bases = np.fromfile(reads_file, np.uint8, count=nb)
        offs = (np.arange(n + 1, dtype=np.int64) * rl)
        ix = movi_amd.MoveIndex.load(idx_dir)
        t0 = time.perf_counter()
        ix.build_ssa(args.rate)
        build_s = time.perf_counter() - t0
        ix.prepare(ix.PREPARE_PML | ix.PREPARE_SA)
        db, do = torch.from_numpy(bases).to(dev), torch.from_numpy(offs).to(dev)
        dsa = torch.empty(nb, dtype=torch.int64, device=dev)
        dp = torch.empty(nb, dtype=torch.int16, device=dev)
        pml_ms = timed(torch, lambda: ix.pml_device(db.data_ptr(), do.data_ptr(), n, nb, dp.data_ptr()), args.steps)
        sa_ms = timed(torch, lambda: ix.sa_entries_device(db.data_ptr(), do.data_ptr(), n, nb, dsa.data_ptr()), args.steps)
        st = ix.last_stats()
        # (the position walk is about 1 % of the call: the call's time stands for the locate walk's)
        row = {"workload": wl_name, "rate": args.rate, "reads": n, "read_len": rl, "rows": ix.desc.r, "build_sa_s": round(build_s, 4),
               "pml_ms": round(pml_ms, 3), "pml_gbases": round(nb / pml_ms / 1e6, 3),
               "sa_entries_ms": round(sa_ms, 3), "sa_entries_gbases": round(nb / sa_ms / 1e6, 4),
               "locate_steps_per_s": round(st.lane_steps / (sa_ms * 1e-3), 1),
               "locate_lines_per_s": round((st.lane_steps + st.fast_forwards) / (sa_ms * 1e-3), 1),
               "pml_lines_per_s": round(pml_rate, 1),
               "walk_mean": round(st.lane_steps / nb, 2),
               "occupancy": round(st.lane_steps / (64.0 * st.wave_steps), 4) if st.wave_steps else None,
               "locate_bytes": ix.info("locate_bytes"), "kernel": ix.last_launch()["kernel"]}
        # the longest walk: the counters are per call, so 256 single-item calls, from the first position of rows spread over the table
        pos = torch.empty(1, dtype=torch.int64, device=dev)
        wmax = 0
        rows_probe = np.linspace(0, ix.desc.r - 1, 256).astype(np.int64)
        for r0 in rows_probe:
            pos[0] = int(r0) << ix.POS_OFFSET_BITS
            ix.locate_device(pos.data_ptr(), 1)
            wmax = max(wmax, int(ix.last_stats().lane_steps))
        row["walk_max_of_256"] = wmax
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        ix.close()


if __name__ == "__main__":
    main()
