"""MEM finding against the count query on the same device-resident batch (movi_mem_device vs movi_count_device, HIP events).

  python tools/mem_bench.py [--steps N] [--only c2|c3]

Workloads: bench.py's c2 pangenome (64 genomes, 14 M rows) with 1 M x 150 bp reads at L = 25 and 31, and its c3 batch,
100 k x 10 kbp (8 % substitutions), at L = 25; interval table K = 12 throughout.  One JSON line per row: milliseconds per
call, Gbases/s of read bases, MEMs found, the ratio to the count query, and the MEM kernel's steps per base and SIMT
efficiency (lane_steps / (64 x wave_steps)) from movi_last_stats."""
import argparse
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    import movi_amd
    dev = torch.device("cuda", 0)
    rows = [("c2", 25), ("c2", 31), ("c3", 25)]
    for wl_name in ("c2", "c3"):
        if args.only and args.only != wl_name:
            continue
        wl = dict(bench.WORKLOADS[wl_name])
        idx_dir, reads_file = bench.ensure_pangenome(wl, 1, 0, lambda: None)
        n, rl = wl["reads"], wl["read_len"]
        bases = np.fromfile(reads_file, np.uint8, count=n * rl)
        offs = (np.arange(n + 1, dtype=np.int64) * rl)
        ix = movi_amd.MoveIndex.load(idx_dir)
        ix.set_option("ftab_k", 12)
        ix.prepare(ix.PREPARE_COUNT)
        db, do = torch.from_numpy(bases).to(dev), torch.from_numpy(offs).to(dev)
        nb = n * rl
        dm = torch.empty(nb * 16, dtype=torch.uint8, device=dev)
        dn = torch.empty(n, dtype=torch.int32, device=dev)
        dmat, dcnt = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        count = lambda: ix.count_device(db.data_ptr(), do.data_ptr(), n, nb, dmat.data_ptr(), dcnt.data_ptr())
        t_count = timed(torch, count, args.steps)
        count_kernel = ix.last_launch()["kernel"]
        for w, L in rows:
            if w != wl_name:
                continue
            mem = lambda: ix.mem_device(db.data_ptr(), do.data_ptr(), n, nb, L, dm.data_ptr(), dn.data_ptr())
            t_mem = timed(torch, mem, args.steps)
            mem()
            st = ix.last_stats()
            found = int(dn.cpu().numpy().view(np.uint32).sum())
            print(json.dumps({
                "workload": wl_name, "reads": n, "read_len": rl, "min_len": L, "ftab_k": 12, "rows": ix.desc.r,
                "mem_ms": round(t_mem, 3), "mem_gbases_s": round(nb / t_mem / 1e6, 2), "mem_kernel": ix.last_launch()["kernel"],
                "count_ms": round(t_count, 3), "count_gbases_s": round(nb / t_count / 1e6, 2), "count_kernel": count_kernel,
                "mem_over_count": round(t_mem / t_count, 2), "mems_found": found,
                "steps_per_base": round(st.lane_steps / nb, 3),
                "simt_efficiency": round(st.lane_steps / (64.0 * st.wave_steps), 3) if st.wave_steps else None,
                "fast_forwards_per_base": round(st.fast_forwards / nb, 3), "scans_per_base": round(st.scans / nb, 3)}), flush=True)
        ix.close()
        del dm


if __name__ == "__main__":
    main()
