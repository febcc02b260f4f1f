// movi_walk_chain.hip -- the walk on the chain rows: pml_kernel_chain's four instantiations (separators or not; PMLs through the register
// packer or as reset masks), in a translation unit of their own (movi_walk.hpp has the kernel and the body it shares with pml_kernel_flatp).
#include "movi_walk.hpp"

namespace movi {

template <int SEP, int RING>
static hipError_t chain_go(const WalkLaunch &L, LaunchInfo *info) {
    auto kern = pml_kernel_chain<SEP, RING>;
    if (L.dyn_lds > 65536) {                               // every kernel that is handed more than 64 KiB of dynamic LDS must opt in first
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.dyn_lds);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(kern, L.grid, L.block, L.dyn_lds, L.stream, L.ix, L.bases, L.offs, L.n, L.out, L.err, L.stats, L.order);
    char name[96];                                         // the name as rocprofv3 prints it
    snprintf(name, sizeof(name), "pml_kernel_chain<%d, %d>", SEP, RING);
    if (info) snprintf(info->kernel, sizeof(info->kernel), "%s", name);
    note_walk_launch(name);
    return hipGetLastError();
}

hipError_t launch_walk_chain(const WalkLaunch &L, LaunchInfo *info) {
    if (!L.stg || L.ahd != 3 || L.psh || L.cls_mode != 0 || L.ix.rows3 == nullptr || (L.ring != 0 && L.ring != 2)) return hipErrorInvalidValue;
    if (L.ring == 2) return L.sep ? chain_go<1, 2>(L, info) : chain_go<0, 2>(L, info);
    return L.sep ? chain_go<1, 0>(L, info) : chain_go<0, 0>(L, info);
}

hipError_t preload_walk_chain() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&pml_kernel_chain<0, 2>));
}

}  // namespace movi
