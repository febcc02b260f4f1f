"""k-mer presence next to the count query and MEM finding on the same device-resident batch (movi_kmer_device vs
movi_count_device vs movi_mem_device, HIP events).

  python tools/kmer_bench.py [--steps N] [--only c2|c3]

Workloads: bench.py's c2 pangenome (64 genomes, 14 M rows) with 1 M x 150 bp reads, and its c3 batch, 100 k x 10 kbp (8 %
substitutions); k = 31 and k = 15, each with the look-ahead at its default ("kmer_lookahead" -1), at the splits k / 3 (the reference's) and k / 2, and off (0);
MEM finding at L = 25; interval table K = 12 throughout.  One JSON line per row: milliseconds per call (one warm-up call,
then the mean of --steps calls between two HIP events), Gbases/s of read bases, k-mers found, the ratios to the count and
MEM queries, and the k-mer kernel's steps per base and SIMT efficiency (lane_steps / (64 x wave_steps)) from movi_last_stats."""
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
        dm = torch.empty(nb * 16, dtype=torch.uint8, device=dev)          # MEMs (16 B per base); the runs (8 B per base) use its front
        dn = torch.empty(n, dtype=torch.int32, device=dev)
        df = torch.empty(n, dtype=torch.int32, device=dev)
        dmat, dcnt = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        count = lambda: ix.count_device(db.data_ptr(), do.data_ptr(), n, nb, dmat.data_ptr(), dcnt.data_ptr())
        t_count = timed(torch, count, args.steps)
        count_kernel = ix.last_launch()["kernel"]
        mem = lambda: ix.mem_device(db.data_ptr(), do.data_ptr(), n, nb, 25, dm.data_ptr(), dn.data_ptr())
        t_mem = timed(torch, mem, args.steps)
        for k in (31, 15):
            for la in (-1, 3, 2, 0):
                ix.set_option("kmer_lookahead", la)
                kmer = lambda: ix.kmer_device(db.data_ptr(), do.data_ptr(), n, nb, k, dm.data_ptr(), dn.data_ptr(), df.data_ptr())
                t_kmer = timed(torch, kmer, args.steps)
                kmer()
                st = ix.last_stats()
                found = int(df.cpu().numpy().view(np.uint32).astype(np.uint64).sum())
                runs = int(dn.cpu().numpy().view(np.uint32).astype(np.uint64).sum())
                print(json.dumps({
                    "workload": wl_name, "reads": n, "read_len": rl, "k": k, "kmer_lookahead": la, "ftab_k": 12, "rows": ix.desc.r,
                    "kmer_ms": round(t_kmer, 3), "kmer_gbases_s": round(nb / t_kmer / 1e6, 2), "kmer_kernel": ix.last_launch()["kernel"],
                    "count_ms": round(t_count, 3), "count_gbases_s": round(nb / t_count / 1e6, 2), "count_kernel": count_kernel,
                    "mem_ms": round(t_mem, 3), "mem_gbases_s": round(nb / t_mem / 1e6, 2), "mem_min_len": 25,
                    "kmer_over_count": round(t_kmer / t_count, 2), "kmer_over_mem": round(t_kmer / t_mem, 2),
                    "kmers_found": found, "kmers_all": n * max(0, rl - k + 1), "runs": runs,
                    "steps_per_base": round(st.lane_steps / nb, 3),
                    "simt_efficiency": round(st.lane_steps / (64.0 * st.wave_steps), 3) if st.wave_steps else None,
                    "fast_forwards_per_base": round(st.fast_forwards / nb, 3), "scans_per_base": round(st.scans / nb, 3)}), flush=True)
        ix.close()
        del dm


if __name__ == "__main__":
    main()
