// Test driver of tests/test_launch_policy_cpu.py: the launch plans of movi_amd/csrc/movi_launch_policy.hpp, printed without a GPU.
// stdin: one case per line (lines that start with '#' are skipped), 28 integers:
//   r idx32 sep rows2 rows3 hints rows2_count   block_threads pml_variant zml_variant count_variant num_cus waves_per_cu seg_len
//   stage_reads out_ring pair_loads zml_ahead deep   n_reads n_bases cm logging have_seg_ws ordered want_mask mode big_batch_cap
// stdout, per case: one line per query kind --
//   pml    v bt wpc dyn_lds stage_lds ring ahead deep pair seg_eligible seg_len(8) seg_len(24)
//   pmlseg dyn_lds stage_lds ring ahd pair of K1 (over max_seg lanes), then of K3 (over n_reads lanes)
//   zml    v bt wpc dyn_lds stage_lds pair ahead seg_eligible k1_flat      (or "zml invalid": no kernel for these options)
//   count  v bt wpc dyn_lds stage_lds pair ahead                           (or "count invalid")
// With the argument "route": the route of a PML call (plan_pml).  A case is the 28 integers (want_mask is not read) and 8 more:
//   want (0 the vector, 1 reset masks, 2 the vector with mask words lent)  aligned fused_expand hints(option) ff_skip park_lanes
//   park_cap (records of the lent queue; -1: none)  pml_via_mask (0: the caller lends nothing -- want 2 is then want 0)
// stdout, one line per case:
//   route KIND seg_first needs_tmp words park_lanes park_grid hint_w ff_skip ahd psh ring     (or "route invalid")
// KIND: vector | mask_native | mask_from_tmp | vector_fused | vector_expand; words: 1 = the call uses the mask words the caller lent.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../movi_amd/csrc/movi_launch_policy.hpp"

using namespace movi;

int main(int argc, char **argv) {
    const bool route_mode = argc > 1 && !strcmp(argv[1], "route");
    const int n_fields = route_mode ? 36 : 28;
    char line[2048];
    while (fgets(line, sizeof(line), stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        long long f[36];
        int n = 0, pos = 0, adv = 0;
        while (n < n_fields && sscanf(line + pos, "%lld%n", &f[n], &adv) == 1) { pos += adv; ++n; }
        if (n != n_fields) { fprintf(stderr, "bad case: %s", line); return 2; }
        TableFacts T;
        T.r = (uint64_t)f[0]; T.idx32 = f[1] != 0; T.sep = f[2] != 0; T.rows2 = f[3] != 0; T.rows3 = f[4] != 0; T.hints = f[5] != 0;
        T.rows2_count = f[6] != 0;
        LaunchCfg c;
        c.block_threads = (int)f[7]; c.pml_variant = (int)f[8]; c.zml_variant = (int)f[9]; c.count_variant = (int)f[10];
        c.num_cus = (int)f[11]; c.waves_per_cu = (int)f[12]; c.seg_len = (int)f[13]; c.stage_reads = (int)f[14]; c.out_ring = (int)f[15];
        c.pair_loads = (int)f[16]; c.zml_ahead = (int)f[17]; c.deep = (int)f[18];
        const uint64_t n_reads = (uint64_t)f[19], n_bases = (uint64_t)f[20];
        const int mode = (int)f[26];
        const bool have_ws = f[23] != 0, ordered = f[24] != 0, want_mask = f[25] != 0, big_cap = f[27] != 0;
        PmlAsk a;
        a.cm = (int)f[21]; a.logging = f[22] != 0; a.have_seg_ws = have_ws; a.ordered = ordered;

        if (route_mode) {
            const int via = (int)f[35];
            a.want = f[28] == 1 ? PmlWant::kMasks : (f[28] == 2 && via != 0) ? PmlWant::kVectorLendsMasks : PmlWant::kVector;
            a.out_aligned = f[29] != 0; a.via_mask = via; a.park_queue = f[34] >= 0; a.park_cap = f[34] >= 0 ? (uint64_t)f[34] : 0;
            c.fused_expand = (int)f[30]; c.hints = (int)f[31]; c.ff_skip = (int)f[32]; c.park_lanes = (int)f[33];
            const PmlRoute R = plan_pml(T, c, n_reads, n_bases, a);
            // (what launch_pml refuses beside the plan's own verdict: a grid of more than 2^31 - 1 blocks)
            if (!R.valid || (n_reads + R.plan.bt - 1) / R.plan.bt > 0x7FFFFFFFull) { printf("route invalid\n"); continue; }
            static const char *const kinds[] = {"vector", "mask_native", "mask_from_tmp", "vector_fused", "vector_expand"};
            printf("route %s %d %d %d %d %" PRIu64 " %u %d %d %d %d\n", kinds[(int)R.kind], (int)R.seg_first, (int)R.needs_tmp, (int)R.lent_masks(),
                   R.park_lanes, R.park_grid, R.hint_w, (int)R.ff_skip, R.ahd, R.psh, R.ring);
            continue;
        }
        const PmlPlan P = plan_pml_walk(T, c, n_reads, n_bases, a, want_mask);
        const uint32_t s8 = call_seg_len(c, n_bases, kSegWavesPml), s24 = call_seg_len(c, n_bases, kSegWavesZml);
        printf("pml %d %d %d %zu %u %d %d %d %d %d %u %u\n", P.v, P.bt, P.wpc, P.dyn_lds, P.stage_lds, (int)P.use_ring, (int)P.use_ahead,
               (int)P.use_deep, (int)P.use_pair, (int)P.seg_eligible, s8, s24);
        const uint64_t max_seg = n_reads + (s8 ? n_bases / s8 : 0) + 1;   // ("seg_len" 0 never reaches the segment plan)
        printf("pmlseg");
        for (const uint64_t lanes : {max_seg, n_reads}) {
            const PmlPlan K = plan_pml_seg(T, c, lanes, big_cap);
            printf(" %zu %u %d %d %d", K.dyn_lds, K.stage_lds, (int)K.use_ring, K.use_deep ? 2 : (K.use_ahead ? 1 : 0), (int)K.use_pair);
        }
        printf("\n");
        const ZmlPlan Z = plan_zml(T, c, mode, n_bases);
        if (!Z.valid) printf("zml invalid\n");
        else printf("zml %d %d %d %zu %u %d %d %d %d\n", Z.v, Z.bt, Z.wpc, Z.dyn_lds, Z.stage_lds, (int)Z.pair, (int)Z.ahead,
                    (int)zml_seg_eligible(c, mode, n_reads, n_bases, have_ws, ordered), (int)zml_seg_k1_flat(T.r, n_bases));
        const ZmlPlan C = plan_count(T, c, mode, n_reads, n_bases);
        if (!C.valid) printf("count invalid\n");
        else printf("count %d %d %d %zu %u %d %d\n", C.v, C.bt, C.wpc, C.dyn_lds, C.stage_lds, (int)C.pair, (int)C.ahead);
    }
    return 0;
}
