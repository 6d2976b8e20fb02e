// Lane-level helpers shared by the MSDA fast paths (msda.hip: fp32 value maps, through msda_fast.h; msda_h16.hip: fp16 / bf16
// value maps): the DPP move, the channel sum over a wavefront half, the reductions over the lane group of one (n, q, m) row, and
// the workgroup -> tile mapping.  Plain device functions, included INSIDE the namespace of the file that uses it, after
// <hip/hip_runtime.h> -- exactly as msda_geom.h and cvt16.h are; msda.hip includes it before msda_fast.h.
#pragma once

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x)
{
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}

// Sum over the 32 lanes of each wavefront half (lane = channel).  After the five steps lanes 16..31 of
// each half hold the half's total; the writer is lane 16 / 48.
__device__ __forceinline__ float half32_sum(float x)
{
    x += dpp_mov<0xB1>(x);    // quad_perm [1,0,3,2]
    x += dpp_mov<0x4E>(x);    // quad_perm [2,3,0,1]
    x += dpp_mov<0x141>(x);   // row_half_mirror
    x += dpp_mov<0x140>(x);   // row_mirror  -> every lane of a 16-lane row holds the row total
    // row_bcast:15 into rows 1 and 3 (row_mask 0xA): lane 15 of the previous row is added to every lane
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x142, 0xA, 0xF, true));
    return x;
}

// Reductions over the L*P logits of one (n, q, m) row, evaluated cooperatively by the LP consecutive threads that own the
// row's samples: by DPP / xor-shuffles when LP is a power of two <= 64 (the DINO case LP = 16 is one DPP row).
__device__ __forceinline__ bool lp_shuffles(int LP) { return (LP & (LP - 1)) == 0 && LP <= 64; }
// sum / max over a lane-aligned group of LP threads (LP a power of two <= 64); every lane of the group gets the result
__device__ __forceinline__ float lp_group_sum(float x, int LP)
{
    if (LP >= 2) x += dpp_mov<0xB1>(x);      // quad_perm [1,0,3,2]
    if (LP >= 4) x += dpp_mov<0x4E>(x);      // quad_perm [2,3,0,1]
    if (LP >= 8) x += dpp_mov<0x141>(x);     // row_half_mirror
    if (LP >= 16) x += dpp_mov<0x140>(x);    // row_mirror
    if (LP >= 32) x += __shfl_xor(x, 16, 64);
    if (LP >= 64) x += __shfl_xor(x, 32, 64);
    return x;
}
__device__ __forceinline__ float lp_group_max(float x, int LP)
{
    if (LP >= 2) x = fmaxf(x, dpp_mov<0xB1>(x));
    if (LP >= 4) x = fmaxf(x, dpp_mov<0x4E>(x));
    if (LP >= 8) x = fmaxf(x, dpp_mov<0x141>(x));
    if (LP >= 16) x = fmaxf(x, dpp_mov<0x140>(x));
    if (LP >= 32) x = fmaxf(x, __shfl_xor(x, 16, 64));
    if (LP >= 64) x = fmaxf(x, __shfl_xor(x, 32, 64));
    return x;
}

// Workgroup -> (n, query tile, m).  Consecutive workgroups take consecutive heads, and the head of a given slot is
// rotated every kHeadRun tiles.  Why: rows of one head are M*128 bytes apart, so with M == 8 all addresses one head
// touches share bits [9:7]; workgroups go round robin to the 8 XCDs, so "blockIdx % 8 == head" pins each XCD to
// ONE such address class for the whole launch.  Measured at the encoder shape, bs 4 (rocprofv3 PMC,
// profiles/r01_msda_fwd_enc_mapping_pmc.txt): with the rotation the L1 traffic and L1 miss traffic are identical
// (91 M accesses, 15.4 M L1->L2 requests), L2 misses go UP 3.5 M -> 4.9 M, yet forward 286 -> 248 us, gather
// 341 -> 320 us, decoder forward 24.7 -> 20.8 us.  Run lengths 2..512 are equivalent in time (242-260 us; longer
// runs re-fetch fewer halo rows across XCDs: HBM reads 540 MB at 64, 418 MB at 256, 356 MB without rotation -- but
// the bench step was 1.5 % slower with 256 or a launch-size dependent length), 1 (adjacent tiles on different XCDs)
// gives 278, 2048 gives 268, >= 8192 is no rotation in practice.  Since a run of 512 tiles (one head per XCD at any
// instant, ~7 different heads per XCD over the launch) is as good as 64, what matters is that no XCD stays married
// to one address class: the classes are not equally fast from every XCD once the accesses leave the L2
// (tools/xcd_class_probe.hip: up to 1.5x between (XCD, class) pairs), every XCD has the same amount of work, and the
// launch ends with the slowest one.  Giving every XCD all 8 heads of a contiguous eighth of the
// tiles was as slow as no rotation (not understood); a head-major copy of the value map (N,M,S,D) brought nothing
// on top.  Speed only -- any bijection is correct.  (Measured on the fp32 kernels; the 16-bit ones take the same mapping.)
constexpr int kHeadRun = 64;
struct Tile {
    int n, q0, m;
};
__device__ __forceinline__ Tile tile_of(int b, int M, int tiles_per_image, int rows_per_block)
{
    Tile t;
    const int r = b / M;
    t.m = (b % M + r / kHeadRun) % M;
    t.q0 = (r % tiles_per_image) * rows_per_block;
    t.n = r / tiles_per_image;
    return t;
}
__device__ __forceinline__ Tile tile_of_block(int M, int tiles_per_image, int rows_per_block)
{
    return tile_of((int)blockIdx.x, M, tiles_per_image, rows_per_block);
}
