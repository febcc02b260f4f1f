"""k-mer occurrences (movi_kmer_occ_device) next to the only way to the same numbers without it -- every k-mer cut out and run
through movi_count_device as a read of its own -- and to the k-mer presence query, on a device-resident batch (HIP events).

  python tools/kmer_occ_bench.py [--repeats N] [--only c2|c3] [--baseline-kmers N]

Workloads: bench.py's c2 pangenome (64 genomes, 14 M rows) with 1 M x 150 bp reads, and its c3 batch, 100 k x 10 kbp (8 %
substitutions); k = 15 and k = 31; interval table K = 12.  Every figure: one warm-up call, then the median of --repeats calls, each
between two HIP events.  The baseline's batch holds k bytes per k-mer, so it is cut from the first reads of the batch only, about
--baseline-kmers k-mers (2^24: 16 M lanes, more than the GPU holds at once), and the occurrence query is timed on those same reads
as well as on the whole batch; the baseline's upload is timed from page-locked memory.  One JSON line per (workload, k):
k-mers/s of the occurrence query (whole batch and subset), of the baseline without and with its upload, the ratios, the presence
query on the same batch, and the occurrence kernel's steps per k-mer and occupancy (lane_steps / (64 x wave_steps))."""
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--baseline-kmers", type=int, default=1 << 24)
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
        docc = torch.empty(nb, dtype=torch.int64, device=dev)
        df = torch.empty(n, dtype=torch.int32, device=dev)
        ds = torch.empty(n, dtype=torch.int64, device=dev)
        druns = torch.empty(nb * 8, dtype=torch.uint8, device=dev)
        dn = torch.empty(n, dtype=torch.int32, device=dev)
        for k in (31, 15):
            per_read = rl - k + 1
            kmers_all = n * per_read
            occ = lambda: ix.kmer_occ_device(db.data_ptr(), do.data_ptr(), n, nb, k, docc.data_ptr(), df.data_ptr(), ds.data_ptr())
            t_occ = timed(torch, occ, args.repeats)
            st = ix.last_stats()
            kernel = ix.last_launch()["kernel"]
            found = int(df.cpu().numpy().view(np.uint32).astype(np.uint64).sum())
            total = int(ds.cpu().numpy().view(np.uint64).sum(dtype=np.uint64))
            pres = lambda: ix.kmer_device(db.data_ptr(), do.data_ptr(), n, nb, k, druns.data_ptr(), dn.data_ptr())
            t_pres = timed(torch, pres, args.repeats)
            # ---- the baseline on the first `sub` reads: their k-mers as reads of their own
            sub = max(1, min(n, args.baseline_kmers // per_read))
            nk = sub * per_read
            dk = db[:sub * rl].view(sub, rl).unfold(1, k, 1).contiguous().view(-1)             # nk * k bytes
            dko = torch.arange(nk + 1, dtype=torch.int64, device=dev) * k
            dmat, dcnt = torch.empty(nk, dtype=torch.int64, device=dev), torch.empty(nk, dtype=torch.int64, device=dev)
            count = lambda: ix.count_device(dk.data_ptr(), dko.data_ptr(), nk, nk * k, dmat.data_ptr(), dcnt.data_ptr())
            t_base = timed(torch, count, args.repeats)
            base_kernel = ix.last_launch()["kernel"]
            hk, hko = dk.cpu().pin_memory(), dko.cpu().pin_memory()

            def count_with_upload():
                dk.copy_(hk, non_blocking=True)
                dko.copy_(hko, non_blocking=True)
                count()
            t_base_up = timed(torch, count_with_upload, args.repeats)
            occ_sub = lambda: ix.kmer_occ_device(db.data_ptr(), do.data_ptr(), sub, sub * rl, k, docc.data_ptr(), df.data_ptr(), ds.data_ptr())
            t_occ_sub = timed(torch, occ_sub, args.repeats)
            # the two ways agree on the subset
            want = torch.where(dmat == k, dcnt, torch.zeros_like(dcnt)).view(sub, per_read)
            same = bool((docc[:sub * rl].view(sub, rl)[:, :per_read] == want).all().item())
            rate = lambda cnt, ms: round(cnt / ms / 1e3, 1)                                    # M k-mers / s
            print(json.dumps({
                "workload": wl_name, "reads": n, "read_len": rl, "k": k, "ftab_k": 12, "rows": ix.desc.r, "kmers": kmers_all,
                "occ_ms": round(t_occ, 3), "occ_mkmers_s": rate(kmers_all, t_occ), "occ_kernel": kernel,
                "kmers_found": found, "sum_of_counts": total,
                "steps_per_kmer": round(st.lane_steps / kmers_all, 3),
                "occupancy": round(st.lane_steps / (64.0 * st.wave_steps), 3) if st.wave_steps else None,
                "subset_reads": sub, "subset_kmers": nk, "occ_subset_ms": round(t_occ_sub, 3), "occ_subset_mkmers_s": rate(nk, t_occ_sub),
                "baseline_ms": round(t_base, 3), "baseline_mkmers_s": rate(nk, t_base), "baseline_kernel": base_kernel,
                "baseline_with_upload_ms": round(t_base_up, 3), "baseline_with_upload_mkmers_s": rate(nk, t_base_up),
                "baseline_upload_bytes": int(nk) * k + (int(nk) + 1) * 8,
                "speedup_over_baseline": round(t_base / t_occ_sub, 2), "speedup_over_baseline_with_upload": round(t_base_up / t_occ_sub, 2),
                "subset_agrees": same,
                "presence_ms": round(t_pres, 3), "presence_mkmers_s": rate(kmers_all, t_pres)}), flush=True)
            del dk, dko, dmat, dcnt, hk, hko
        ix.close()
        del docc, druns


if __name__ == "__main__":
    main()
