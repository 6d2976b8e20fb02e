// What the two arithmetics of the decoder self-attention (self_attn.hip: fp32; self_attn_h16.hip: 16-bit operands) share: the
// 32 x 32 tile classes of the byte mask, the wave-uniform scan over them, the accumulator's row map and the workspace layout
// (delta (B, H, Lq) fp32, then the (nqt, nkt) class bytes).  Included INSIDE the namespace of the file that uses it, after
// <hip/hip_runtime.h> and "common.h".
#pragma once

constexpr int kD = 32;                       // head dimension
constexpr int kTile = 32;                    // rows of an MFMA tile: queries per wave, keys per staged tile
constexpr int kWaves = 2, kThreads = 64 * kWaves;
constexpr float kLog2e = 1.44269504088896340736f;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Tiles {
    const uint8_t *cls;        // (nqt, nkt) tile classes, NULL without a mask
    int nqt, nkt;              // 32-row tiles of queries / keys
};

// register r of a 32 x 32 accumulator in lane half h holds this row (the column is the lane & 31)
__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ int tile_class(const Tiles &L, int qt, int kt)
{
    if (qt >= L.nqt || kt >= L.nkt) return 0;
    return L.cls ? (int)L.cls[qt * L.nkt + kt] : 2;
}

__global__ __launch_bounds__(64) void sattn_class_kernel(const uint8_t *__restrict__ mask, int Lq, int Lk, int nkt,
                                                         uint8_t *__restrict__ cls)
{
    const int kt = blockIdx.x, qt = blockIdx.y, lane = threadIdx.x;
    const int q = qt * kTile + (lane >> 1), k0 = kt * kTile + 16 * (lane & 1);
    bool open = false, blocked = false;
    if (q < Lq) {
        for (int j = 0; j < 16; ++j) {
            if (k0 + j >= Lk) break;
            const bool b = mask[(int64_t)q * Lk + k0 + j] != 0;
            open |= !b;
            blocked |= b;
        }
    }
    const bool any_open = __ballot(open) != 0, any_blocked = __ballot(blocked) != 0;
    if (lane == 0) cls[qt * nkt + kt] = any_open ? (any_blocked ? 1 : 2) : 0;
}

// The classes of 64 consecutive tiles at a time, one tile per lane, as wave-uniform bit masks: which tiles the workgroup stages
// (a tile open for either wave) and which this wave multiplies.  BY_KEY walks the key tiles of the query tiles (a0, a0 + 1),
// otherwise the query tiles of the key tiles (a0, a0 + 1).
template <bool BY_KEY>
struct TileScan {
    uint64_t open, mine, mixed;
    int base, n, a0, wv;
    __device__ __forceinline__ TileScan(const Tiles &L, int a0_, int wv_) : n(BY_KEY ? L.nkt : L.nqt), a0(a0_), wv(wv_) { load(L, 0); }
    __device__ __forceinline__ void load(const Tiles &L, int b)
    {
        base = b;
        const int t = b + (threadIdx.x & 63);
        const int c0 = BY_KEY ? tile_class(L, a0, t) : tile_class(L, t, a0);
        const int c1 = BY_KEY ? tile_class(L, a0 + 1, t) : tile_class(L, t, a0 + 1);
        const int cm = wv ? c1 : c0;
        open = __ballot((c0 | c1) != 0);
        mine = __ballot(cm != 0);
        mixed = __ballot(cm == 1);
    }
    // the first tile >= t that the workgroup stages, n when there is none
    __device__ __forceinline__ int next(const Tiles &L, int t)
    {
        while (t < n) {
            if (t >= base + 64) load(L, t & ~63);
            const uint64_t m = open >> (t - base);
            if (m) return t + __builtin_ctzll(m);
            t = base + 64;
        }
        return n;
    }
    // this wave's class of tile t of the loaded 64
    __device__ __forceinline__ int cls(int t) const
    {
        const int s = t - base;
        return ((mine >> s) & 1) ? (((mixed >> s) & 1) ? 1 : 2) : 0;
    }
};

size_t delta_bytes(int batch, int heads, int len_q) { return (((size_t)batch * heads * len_q * sizeof(float)) + 15) & ~(size_t)15; }

// the sizes both arithmetics accept (the caller has checked that the block is not NULL and head_dim)
template <typename P>
int sizes_ok(const P &p, const char *op)
{
    SEMIDETR_REQUIRE(p.batch > 0 && p.heads > 0 && p.len_q > 0 && p.len_k > 0, SEMIDETR_E_BADARG,
                     "%s: bad sizes (B=%d H=%d Lq=%d Lk=%d)", op, p.batch, p.heads, p.len_q, p.len_k);
    SEMIDETR_REQUIRE(p.scale == p.scale, SEMIDETR_E_BADARG, "%s: scale is NaN", op);
    SEMIDETR_REQUIRE((int64_t)p.batch * p.heads <= 65535 && (int64_t)p.len_q * p.len_k < ((int64_t)1 << 40) &&
                         (int64_t)p.len_q < (1 << 24) && (int64_t)p.len_k < (1 << 24) &&
                         (int64_t)((p.len_q + 31) / 32) * ((p.len_k + 31) / 32) < ((int64_t)1 << 31) &&
                         (int64_t)p.batch * p.heads * (p.len_q > p.len_k ? p.len_q : p.len_k) * kD < ((int64_t)1 << 40),
                     SEMIDETR_E_TOOLARGE, "%s: too large (B * H <= 65535, Lq and Lk < 2^24)", op);
    return SEMIDETR_OK;
}

// delta and the class bytes in the workspace; the tile counts
template <typename P>
void carve(const P &p, void *workspace, Tiles &t, float *&delta)
{
    t.nqt = (p.len_q + kTile - 1) / kTile;
    t.nkt = (p.len_k + kTile - 1) / kTile;
    delta = static_cast<float *>(workspace);
    t.cls = p.mask ? reinterpret_cast<uint8_t *>(workspace) + delta_bytes(p.batch, p.heads, p.len_q) : nullptr;
}

int launch_class(hipStream_t st, const Tiles &t, const uint8_t *mask, int len_q, int len_k)
{
    if (!t.cls) return SEMIDETR_OK;
    hipLaunchKernelGGL(sattn_class_kernel, dim3(t.nkt, t.nqt), dim3(64), 0, st, mask, len_q, len_k, t.nkt, const_cast<uint8_t *>(t.cls));
    return semidetr::launch_status("sattn_class_kernel");
}
