// Reduction plans of the three gradient entry points: how large an LDS table one workgroup gets.
// Host-only, plain C++ (no HIP headers), so that tests/test_reduction_plan.py can compile it with g++ and check
// which side of each switch the boundary tests in tests/test_gpu_reduction_boundaries.py sit on.
#pragma once
#include <cstddef>

namespace nvdr_plan {

// ---- texture gradient (texture.hip, k_tex_grad / k_tex_grad_lean) ----------------------------------------------------------
// LDS patch table: as many power-of-two patches of 16 texels as fit in 26 KiB (at most 512), so that six workgroups share a CU
// (the kernel is latency bound: occupancy matters more than table size); none (direct atomics) when even 16 patches do not fit,
// and none beyond the 32-bit key format of PatchTable::key_of (width up to 32768, height x faces up to 65536 texels).
inline std::size_t tex_grad_lds(int groups, int C) {
    return (std::size_t)groups * (8 + 64 * (std::size_t)C) + 16;       // 16 texels x C 32-bit sums + key 4 B + used-list entry 4 B per patch
}
inline int tex_grad_groups(int C, int tex_w, int tex_h, bool cube) {
    int groups = 512;
    while (groups >= 16 && tex_grad_lds(groups, C) > 26 * 1024) groups >>= 1;
    if (groups < 16 || tex_w > 32768 || (long long)tex_h * (cube ? 6 : 1) > 65536) groups = 0;
    return groups;
}

// ---- interpolate gradient (interpolate.hip, k_interp_grad) -----------------------------------------------------------------
// LDS vertex table: as many power-of-two slots as fit in 20 KiB (8 workgroups per CU), at most 512, at least 32 (then above
// 20 KiB); vertices too wide for even 32 slots in 64 KiB (A >= 256) go without one: every contribution is an f32 atomic.
inline std::size_t interp_grad_lds(int slots, int A) {
    return (std::size_t)slots * (8 * (std::size_t)A + 6) + 16;          // sums + key + used-list entry per slot
}
inline int interp_grad_slots(int A) {
    int slots = 512;
    while (slots > 32 && interp_grad_lds(slots, A) > 20 * 1024) slots >>= 1;
    if (interp_grad_lds(slots, A) > 64 * 1024) slots = 0;
    return slots;
}

// ---- fused interpolate + rasterize gradient (backward_fused.hip, k_interp_raster_grad) --------------------------------------
// A + 3 components per vertex (attributes, x, y, w); as many power-of-two slots as fit in 32 KiB (four 8-wave workgroups per CU),
// at most 512; none (plain atomics) for vertices too wide for even 32 slots in 64 KiB.
inline std::size_t fused_grad_lds(int slots, int A) {
    return (std::size_t)slots * (8 * (std::size_t)(A + 3) + 6) + 16;    // sums, key, used-list entry, header
}
inline int fused_grad_slots(int A) {
    int slots = 512;
    while (slots > 32 && fused_grad_lds(slots, A) > 32 * 1024) slots >>= 1;
    if (fused_grad_lds(slots, A) > 64 * 1024) slots = 0;
    return slots;
}

}  // namespace nvdr_plan
