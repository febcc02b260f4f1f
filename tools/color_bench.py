"""Movi Color on the bench inputs: writes profiles/color_bench.txt.

  * the colour builder on the c2 index (one document per genome of the pangenome): seconds of the walk, the sorts, the numbering on the
    host and the write of doc_sets_flat.bin (movi_index_info "color_*_seconds"), the chunks it took, the mean set size;
  * `--multi-classify` (movi_multi_classify_device, counters in the handle's scratch) on the c2 and c3 read batches, Gbases/s, beside
    the plain PML walk (movi_pml_device) of the same run.

Usage: python tools/color_bench.py [--steps 5] [--reads N] [--out profiles/color_bench.txt]   (needs the GPU and bench.py's cached inputs)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_bench.txt"))
    a = ap.parse_args()
    import torch
    import bench
    import movi_amd
    lines = []
    for cfg in ("c2", "c3"):
        wl = dict(bench.WORKLOADS[cfg])
        index_dir, reads_file = bench.ensure_pangenome(wl, 1, 0, lambda: None)
        rl = wl["read_len"]
        nr_take = min(wl["reads"], a.reads or (1000000 if rl < 1024 else 10000))
        bases = np.fromfile(reads_file, np.uint8, count=nr_take * rl)
        offs = np.arange(nr_take + 1, dtype=np.uint64) * np.uint64(rl)
        n_genomes = int(bench.pg_of(wl)["genomes"])
        gpu = movi_amd.MoveIndex.load(index_dir)
        n = gpu.desc.length
        ends = [(n - 1) * (g + 1) // n_genomes for g in range(n_genomes)]      # genomes of equal length, reverse complements included
        t = time.perf_counter()
        gpu.build_colors(ends)
        build_s = time.perf_counter() - t
        path = os.path.join(index_dir, "doc_sets_flat.bench.bin")
        t = time.perf_counter()
        gpu.save_colors(path)
        write_s = time.perf_counter() - t
        os.remove(path)
        flat, inds, ns, _ = gpu.colors()
        mean_set = float(flat[inds.astype(np.int64)].mean())
        if cfg == "c2":
            lines.append("builder on %s (n = %d, r = %d, %d documents): %.3f s = walk %.3f + sort %.3f (%d chunk(s)) + numbering on the host %.3f "
                         "(+ the sampled suffix array where none was attached); write %.3f s; flat_colors %d entries, mean set size %.2f"
                         % (cfg, n, gpu.desc.r, n_genomes, build_s, gpu.info("color_walk_seconds"), gpu.info("color_sort_seconds"),
                            gpu.info("color_chunks"), gpu.info("color_number_seconds"), write_s, len(flat), mean_set))
        gpu.prepare(gpu.PREPARE_PML | gpu.PREPARE_COLOR)
        dev = torch.device("cuda", 0)
        db = torch.from_numpy(np.ascontiguousarray(bases)).to(dev)
        do = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).to(dev)
        nr, nb = len(offs) - 1, int(offs[-1])
        dp = torch.zeros(nb, dtype=torch.int16, device=dev)
        dout = torch.zeros(nr * 24, dtype=torch.uint8, device=dev)
        pml_s = timed(lambda: gpu.pml_device(db.data_ptr(), do.data_ptr(), nr, nb, dp.data_ptr()), a.steps)
        mc_s = timed(lambda: gpu.multi_classify_device(db.data_ptr(), do.data_ptr(), nr, nb, 1, dout.data_ptr()), a.steps)
        lines.append("%s: %d reads, %d bases: --multi-classify %.2f Gbases/s (%s), plain PML %.2f Gbases/s; mean set size %.2f, %d species"
                     % (cfg, nr, nb, nb / mc_s / 1e9, gpu.last_launch()["kernel"], nb / pml_s / 1e9, mean_set, ns))
        gpu.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
