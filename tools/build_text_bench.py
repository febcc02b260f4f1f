"""Measures `movi build --gpu-build`'s engine (movi_build_from_text / movi_rlbwt_from_text) and writes profiles/build_text.txt:

  1. c2's text (tools/build_index pangenome ... text-only, the line bench.prepare_inputs uses): per-stage seconds, doubling rounds, peak
     device bytes and the whole call, twice in one process; beside it the seconds of the CPU constructor (tools/build_index) on the same
     text on the same machine, and the two images compared byte for byte.
  2. one text past 2^31 characters (a synthetic pangenome of 2^31 + 2^26) with verify = 1: seconds, memory, the verifier's verdict and
     the sanity of the arrays.  No CPU reference exists at that size.

python tools/build_text_bench.py [--out FILE] [--skip-c2] [--skip-big] [--work DIR]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOOL = os.path.join(ROOT, "tools", "build_index")
BIG = dict(anc=(2 ** 31 + 2 ** 26) // 128, genomes=64, snp=0.01, seed=21)      # 64 genomes + reverse complements = 2^31 + 2^26 characters


def pangenome(pg, mode, out_dir, text_only):
    args = [TOOL, "pangenome", str(pg["anc"]), str(pg["genomes"]), str(pg["snp"]), str(pg["seed"]), str(mode), out_dir]
    t0 = time.time()
    subprocess.check_call(args + (["text-only"] if text_only else []), stderr=subprocess.DEVNULL)
    return time.time() - t0


def stages(st):
    return ", ".join("%s %.3f" % (k, v) for k, v in st.seconds.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_text.txt"))
    ap.add_argument("--skip-c2", action="store_true")
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    import bench
    import movi_amd
    work = a.work or tempfile.mkdtemp(prefix="movi_text_bench")
    os.makedirs(work, exist_ok=True)
    lines = ["movi_build_from_text / movi_rlbwt_from_text on one MI355X (tools/build_text_bench.py).  Seconds per stage: upload | suffix sort |",
             "BWT and runs | LCP | thresholds | verify; `call` is the whole Python call, the table builder and the copy of the image included.", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, "w") as f:                                  # (kept current: a later step may be cut short)
            f.write("\n".join(lines) + "\n")

    if not a.skip_c2:
        pg = bench.PG_C2
        d = os.path.join(work, "c2")
        t_text = pangenome(pg, 6, d, True)
        text = np.fromfile(os.path.join(d, "text.bin"), np.uint8)
        say("1. c2's text: tools/build_index pangenome %d %d %g %d 6 DIR text-only -- %d characters (text made in %.1f s)"
            % (pg["anc"], pg["genomes"], pg["snp"], pg["seed"], text.size, t_text))
        img = None
        for k in range(2):
            stats = []
            t0 = time.time()
            img = movi_amd.build_image_from_text(text, 6, stats=stats)
            call = time.time() - t0
            st = stats[0]
            say("   GPU call %d: %.2f s call | %s | %d rounds, %d runs, peak %d device bytes (%.2f per character; plan %d)%s"
                % (k, call, stages(st), st.rounds, st.original_r, st.device_bytes, st.device_bytes / st.n_positions,
                   movi_amd.text_device_bytes(text.size), "   (first call of the process: runtime start-up and code loading included)" if k == 0 else ""))
        cpu_dir = os.path.join(work, "c2_cpu")
        t_cpu = pangenome(pg, 6, cpu_dir, False)
        want = open(os.path.join(cpu_dir, "index.movi"), "rb").read()
        say("   CPU constructor (tools/build_index, one thread, this machine): %.1f s for the same command without text-only, %.1f s of it the text"
            " -> %.1f s of construction" % (t_cpu, t_text, t_cpu - t_text))
        say("   images: %d and %d bytes, %s" % (len(img), len(want), "EQUAL byte for byte" if img == want else "DIFFERENT"))
        say("")
        del text, img, want
        shutil.rmtree(d, ignore_errors=True)
        shutil.rmtree(cpu_dir, ignore_errors=True)
    if not a.skip_big:
        d = os.path.join(work, "big")
        t_text = pangenome(BIG, 6, d, True)
        text = np.fromfile(os.path.join(d, "text.bin"), np.uint8)
        shutil.rmtree(d, ignore_errors=True)
        say("2. past 2^31: tools/build_index pangenome %d %d %g %d 6 DIR text-only -- %d characters = 2^31 + %d (text made in %.1f s)"
            % (BIG["anc"], BIG["genomes"], BIG["snp"], BIG["seed"], text.size, text.size - 2 ** 31, t_text))
        t0 = time.time()
        heads, lens, thr, st = movi_amd.rlbwt_from_text(text, verify=True)
        call = time.time() - t0
        say("   movi_rlbwt_from_text, verify = 1: %.2f s call | %s | %d rounds, %d runs (n / r = %.2f), peak %d device bytes (%.2f per character; plan %d)"
            % (call, stages(st), st.rounds, st.original_r, st.n_positions / st.original_r, st.device_bytes, st.device_bytes / st.n_positions,
               movi_amd.text_device_bytes(text.size)))
        counts = sum(np.bincount(text[i:i + (1 << 26)], minlength=256) for i in range(0, text.size, 1 << 26))
        by_head = np.bincount(heads, weights=lens.astype(np.float64), minlength=256).astype(np.int64)
        sane = (int(lens.sum()) == text.size + 1 and bool((heads[1:] != heads[:-1]).all()) and int(thr.max()) <= text.size and
                bool((by_head[1:] == counts[1:]).all()) and by_head[0] == 1)
        say("   verifier: %s.  Arrays: lengths add up to N, neighbouring heads differ, every character as often in the BWT as in the text,"
            " thresholds within the text: %s" % ("PASSED (stats.verified = 1)" if st.verified == 1 else "did not run", "yes" if sane else "NO"))
        say("   This is the only evidence above 2^31: no CPU reference exists at that size (the host constructor and the oracle are 32-bit"
            " signed and stop at 2^31 characters).")
    if not a.work:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
