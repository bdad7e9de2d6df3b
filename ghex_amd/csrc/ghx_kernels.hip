// ghx_kernels.hip — gfx950 (CDNA4) pack / unpack kernels for the halo path.
//
// One launch covers every (field, iteration space, buffer) of a plan. Work is cut in the
// BUFFER's byte space: a workgroup tile is tile_bytes (default 8 KiB) of one segment's buffer
// range, so the buffer side is always a linear, fully coalesced 16 B/lane stream, and the field
// side is linear within each contiguous row. Each lane decodes its buffer byte position into
// (row, column) and the row into field coordinates with magic-number division, so no launch
// depends on the shape of an iteration space: face, edge and corner spaces of all fields share
// the one grid (the reference launches one kernel per iteration space per field,
// include/ghex/structured/pack_kernels.hpp:216-241, with a per-element 32-bit divide chain,
// include/ghex/structured/field_utils.hpp:128-159).
//
// Vector width per segment: the widest W in {16,8,4,2,1} bytes dividing the row length, the
// row offsets/strides (planner) and the runtime base pointers (checked per tile here), so the
// same plan is correct for any pointer alignment. No MFMA: this path is pure data movement.
// Four vectors in flight per lane per loop trip (U = 4; 2 and 8 measured slower).
//
// The variants that lost their A/Bs in rounds 1-2 (paired / interleaved / LDS-staged short rows,
// software-pipelined and chunked self tiles, non-temporal policies) were removed from this file
// in round 3; their code and numbers are in tools/kernel_variants_r02.hip.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>
#include <vector>

#include "ghx_addr.hpp"
#include "ghx_internal.hpp"

namespace ghx
{
tuning g_tune{};

// Per-launch kernel timing (ghx_launch_timing): while enabled on a thread, every launch from that
// thread goes through hipExtLaunchKernelGGL with a start and a stop event, which the runtime
// records at the kernel's own begin and end (the interval rocprofv3's kernel trace reports),
// not around the host call. Eager launches only (not during stream capture).
thread_local std::vector<std::pair<hipEvent_t, hipEvent_t>>* t_timing = nullptr;

template<typename K, typename... A>
static void launch(K kernel, uint32_t grid, hipStream_t s, A... args)
{
    if (t_timing)
    {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess)
        {
            hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, e0, e1, 0, args...);
            t_timing->emplace_back(e0, e1);
            return;
        }
        if (e0) (void)hipEventDestroy(e0);
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, args...);
}

namespace
{
constexpr int kU = 4;  // vectors in flight per lane per loop trip

template<int W>
struct vec_t;
template<>
struct vec_t<16>
{
    using type = unsigned __attribute__((ext_vector_type(4)));
};
template<>
struct vec_t<8>
{
    using type = unsigned __attribute__((ext_vector_type(2)));
};
template<>
struct vec_t<4>
{
    using type = unsigned;
};
template<>
struct vec_t<2>
{
    using type = unsigned short;
};
template<>
struct vec_t<1>
{
    using type = unsigned char;
};

// Fields and buffers are device (global) memory: address-space-1 pointers make the compiler
// emit global_load/global_store instead of flat_* (no aperture check, and no lgkmcnt coupling
// that forces every store to wait for all outstanding loads).
#define GHX_GLOBAL __attribute__((address_space(1)))

template<typename V>
__device__ __forceinline__ V vload(const char* p)
{
    return *(const GHX_GLOBAL V*)(p);
}

template<typename V>
__device__ __forceinline__ void vstore(char* p, V v)
{
    *(GHX_GLOBAL V*)(p) = v;
}

// Field-side accesses under the segment's cache policy (seg_s::fpol, uniform per tile; knob
// "short_pol" sets it on short-row segments): bit 0 = non-temporal load, bit 1 = store with sc1
// (gfx950 cache-policy bit; the compiler exposes no builtin for it, hence the asm). Measured
// neutral-to-worse warm; kept for the cold-cache A/Bs.
template<typename V>
__device__ __forceinline__ V fload(const char* p, uint32_t pol)
{
    if (pol & 1u) return __builtin_nontemporal_load((const GHX_GLOBAL V*)(p));
    return vload<V>(p);
}

template<typename V>
__device__ __forceinline__ void fstore(char* p, V v, uint32_t pol)
{
    if constexpr (sizeof(V) == 16)
    {
        if (pol & 2u)
        {
            asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
            return;
        }
    }
    else if constexpr (sizeof(V) == 8)
    {
        if (pol & 2u)
        {
            asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
            return;
        }
    }
    else if constexpr (sizeof(V) == 4)
    {
        if (pol & 2u)
        {
            asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
            return;
        }
    }
    vstore<V>(p, v);
}

// The short form (seg_s::amode 1 / 2, planner short_addressing): the offset of buffer position
// p RELATIVE to s.field_off, in 32 bits. Every product has both operands below 2^24 and a result
// below 2^32, so the full-rate v_mul_u32_u24 is exact; the last outer coordinate is the quotient
// itself (rows < ext[0]*ext[1](*ext[2])), so NDIV = n_outer - 1 divisions (at least one).
template<int NDIV>
__device__ __forceinline__ uint32_t field_offset_f(const seg_s& s, uint32_t p)
{
    const uint32_t row = fastdiv(p, s.mag_row);
    uint32_t off = p - __umul24(row, s.row_bytes);
    const uint32_t q0 = fastdiv(row, s.mag_ext[0]);
    off += __umul24(row - __umul24(q0, s.ext[0]), uint32_t(s.stride[0]));
    if constexpr (NDIV == 1)
        off += __umul24(q0, uint32_t(s.stride[1]));
    else
    {
        const uint32_t q1 = fastdiv(q0, s.mag_ext[1]);
        off += __umul24(q0 - __umul24(q1, s.ext[1]), uint32_t(s.stride[1]));
        off += __umul24(q1, uint32_t(s.stride[2]));
    }
    return off;
}

__device__ __forceinline__ int64_t load_lid(const seg_u& s, uint32_t i)
{
    if (s.lid64) return ((const GHX_GLOBAL int64_t*)(s.lids))[i];
    return ((const GHX_GLOBAL int32_t*)(s.lids))[i];
}

template<typename Seg>
__device__ __forceinline__ int64_t field_offset(const Seg& s, uint32_t p);
template<>
__device__ __forceinline__ int64_t field_offset<seg_s>(const seg_s& s, uint32_t p)
{
    return field_offset_s(s, p);
}

// Copy one tile [start, end) of a segment. Lane-linear in buffer space: lanes of a wave touch
// consecutive W-byte vectors of the buffer; kU independent vectors in flight per lane.
// AM: the segment's offset arithmetic (seg_s::amode): 0 general; 1 / 2 the short form, field
// addressed as (field + field_off) + a 32-bit offset.
template<bool PACK, int W, typename Seg, int AM = 0, int kU = ghx::kU>
__device__ __forceinline__ void copy_tile(const Seg& s, char* __restrict__ field,
                                          char* __restrict__ buf, uint32_t start, uint32_t end)
{
    using V = typename vec_t<W>::type;
    const uint32_t tid = threadIdx.x;
    const uint32_t pol = s.fpol;
    if constexpr (AM != 0) field += s.field_off;
    for (uint32_t base = start + tid * W; base < end; base += kU * kBlock * W)
    {
        V v[kU];
        using off_t = std::conditional_t<AM == 0, int64_t, uint32_t>;
        off_t fo[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * W;
            if constexpr (AM == 0)
            {
                if (p < end) fo[u] = field_offset<Seg>(s, p);
            }
            else if (p < end)
                fo[u] = field_offset_f<AM>(s, p);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * W;
            if (p < end)
            {
                if (PACK) v[u] = fload<V>(field + fo[u], pol);
                else v[u] = vload<V>(buf + p);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * W;
            if (p < end)
            {
                if (PACK) vstore<V>(buf + p, v[u]);
                else fstore<V>(field + fo[u], v[u], pol);
            }
        }
    }
}

// The unpack of a tile of several steps (unpack plans with long-row tiles above 8 KiB,
// g_tune.unpack_tile_bytes), software-pipelined: each lane issues the buffer loads of step k+1
// before the field stores of step k, so a workgroup keeps its reads in flight while its writes
// drain (the unpack is bound by its writes, §4.4 of DESIGN.md); kP vectors per lane per step.
template<int W, typename Seg>
__device__ __forceinline__ void unpack_tile_pipelined(const Seg& s, char* __restrict__ field,
                                                      char* __restrict__ buf, uint32_t start,
                                                      uint32_t end)
{
    using V = typename vec_t<W>::type;
    constexpr int kP = 2;
    const uint32_t pol = s.fpol;
    const uint32_t step = kP * kBlock * W;
    uint32_t base = start + threadIdx.x * W;
    if (base >= end) return;
    V v[kP];
    int64_t fo[kP];
#pragma unroll
    for (int u = 0; u < kP; ++u)
    {
        const uint32_t p = base + u * kBlock * W;
        if (p < end)
        {
            fo[u] = field_offset<Seg>(s, p);
            v[u] = vload<V>(buf + p);
        }
    }
    for (;;)
    {
        const uint32_t nb = base + step;
        const bool more = nb < end;
        V w[kP];
        int64_t fn[kP];
        if (more)
        {
#pragma unroll
            for (int u = 0; u < kP; ++u)
            {
                const uint32_t p = nb + u * kBlock * W;
                if (p < end)
                {
                    fn[u] = field_offset<Seg>(s, p);
                    w[u] = vload<V>(buf + p);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kP; ++u)
            if (base + u * kBlock * W < end) fstore<V>(field + fo[u], v[u], pol);
        if (!more) break;
        base = nb;
        for (int u = 0; u < kP; ++u)  // register renaming (fully unrolled by the compiler)
        {
            v[u] = w[u];
            fo[u] = fn[u];
        }
    }
}

// Unstructured rows of L = 4 or 8 bytes with run detection (seg_u::runs): lane t of a wave moves
// the 16-B buffer chunk [p, p+16) = rows r0 .. r0+K-1 (K = 16/L). It loads the chunk's K lids
// with one vector load and tests whether they form a run (lid[j] = lid[0] + j): then the K rows
// are 16 contiguous field bytes and move as ONE 16-B field access; otherwise as K L-byte
// accesses assembled into the same 16-B buffer vector. The buffer side is a lane-linear
// 16 B/lane stream either way (the one-row-per-lane path moves 4-8 B per lane instruction).
// A wave whose lids are all runs issues the per-row instructions with an empty EXEC mask, which
// the hardware skips; mixed waves execute both, masked. Field accesses of a run are only
// L-aligned: the HSA runtime runs kernels in unaligned-access mode, so a 16-B access at a 4-B
// aligned address is legal (split by the TA where it crosses a line).
using v4_a4 = unsigned __attribute__((ext_vector_type(4), aligned(4)));

template<int K>
__device__ __forceinline__ void load_lids(const seg_u& s, uint32_t r0, int64_t (&l)[K])
{
    if (s.lid64)
    {
        const GHX_GLOBAL vec_t<16>::type* p =
            (const GHX_GLOBAL vec_t<16>::type*)((const int64_t*)(s.lids) + r0);
#pragma unroll
        for (int j = 0; j < K; j += 2)
        {
            const auto q = p[j / 2];
            l[j] = int64_t(uint64_t(q.x) | (uint64_t(q.y) << 32));
            l[j + 1] = int64_t(uint64_t(q.z) | (uint64_t(q.w) << 32));
        }
    }
    else if constexpr (K == 2)
    {
        const auto q = *(const GHX_GLOBAL vec_t<8>::type*)((const int32_t*)(s.lids) + r0);
        l[0] = int32_t(q.x);
        l[1] = int32_t(q.y);
    }
    else
    {
        const auto q = *(const GHX_GLOBAL vec_t<16>::type*)((const int32_t*)(s.lids) + r0);
        l[0] = int32_t(q.x);
        l[1] = int32_t(q.y);
        l[2] = int32_t(q.z);
        l[3] = int32_t(q.w);
    }
}

template<int L>
__device__ __forceinline__ vec_t<16>::type assemble(const typename vec_t<L>::type (&w)[16 / L])
{
    if constexpr (L == 8) return vec_t<16>::type{w[0].x, w[0].y, w[1].x, w[1].y};
    else return vec_t<16>::type{w[0], w[1], w[2], w[3]};
}

template<int L>
__device__ __forceinline__ void split(vec_t<16>::type v, typename vec_t<L>::type (&w)[16 / L])
{
    if constexpr (L == 8)
    {
        w[0] = vec_t<8>::type{v.x, v.y};
        w[1] = vec_t<8>::type{v.z, v.w};
    }
    else
    {
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
}

template<bool PACK, int L>
__device__ __forceinline__ void copy_runs(const seg_u& s, char* __restrict__ field,
                                          char* __restrict__ buf, uint32_t start, uint32_t end)
{
    using V = typename vec_t<16>::type;
    using R = typename vec_t<L>::type;
    constexpr int K = 16 / L;
    const uint32_t pol = s.fpol;
    for (uint32_t base = start + threadIdx.x * 16; base < end; base += kU * kBlock * 16)
    {
        int64_t fo[kU][K];
        uint32_t full = 0, run = 0;  // bit u: chunk u holds K rows / ... that form a run
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * 16;
            if (p >= end) continue;
            const uint32_t r0 = p / L;
            int64_t l[K];
            if (p + 16 <= end)
            {
                full |= 1u << u;
                load_lids<K>(s, r0, l);
                bool c = true;
#pragma unroll
                for (int j = 1; j < K; ++j) c = c && l[j] == l[0] + j;
                if (c) run |= 1u << u;
            }
            else
            {
#pragma unroll
                for (int j = 0; j < K; ++j) l[j] = p + j * L < end ? load_lid(s, r0 + j) : 0;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) fo[u][j] = s.field_off + l[j] * L;  // index stride = L (planner)
        }
        V v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * 16;
            if (p >= end || !(full >> u & 1u)) continue;
            if (PACK)
            {
                if (run >> u & 1u)
                {
                    const v4_a4 x = fload<v4_a4>(field + fo[u][0], pol);
                    v[u] = V{x.x, x.y, x.z, x.w};
                }
                else
                {
                    R w[K];
#pragma unroll
                    for (int j = 0; j < K; ++j) w[j] = fload<R>(field + fo[u][j], pol);
                    v[u] = assemble<L>(w);
                }
            }
            else
                v[u] = vload<V>(buf + p);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * 16;
            if (p >= end) continue;
            if (!(full >> u & 1u))
            {
                // segment tail: fewer than K rows left, row by row
#pragma unroll
                for (int j = 0; j < K; ++j)
                {
                    if (p + j * L >= end) break;
                    if (PACK) vstore<R>(buf + p + j * L, fload<R>(field + fo[u][j], pol));
                    else fstore<R>(field + fo[u][j], vload<R>(buf + p + j * L), pol);
                }
                continue;
            }
            if (PACK)
                vstore<V>(buf + p, v[u]);
            else if (run >> u & 1u)
                fstore<v4_a4>(field + fo[u][0], v4_a4{v[u].x, v[u].y, v[u].z, v[u].w}, pol);
            else
            {
                R w[K];
                split<L>(v[u], w);
#pragma unroll
                for (int j = 0; j < K; ++j) fstore<R>(field + fo[u][j], w[j], pol);
            }
        }
    }
}

__device__ __forceinline__ int ptr_wlog2(uint64_t p)
{
    return __builtin_ctzll(p | 16ull);  // log2 of the largest power of two (<= 16) dividing p
}

// Unstructured tile, general path (rows that are not 4/8-B runs, e.g. config 5's 64-B
// levels-first rows): all kU index loads of a lane, then all kU value loads, are issued
// together. Written branch-free per vector: the uniform choices (index width, row mode, cache
// policy) are hoisted out of the per-vector code, and a vector position past the tile's end is
// clamped to the tile's last vector, which moves the same bytes again (a duplicate store of
// identical bytes by another lane of this workgroup). Per-vector branches made the compiler wait
// for each index load before issuing the next (s_waitcnt vmcnt(0) inside every branch): four
// dependent round trips per lane instead of one.
template<bool PACK, int W, int kU>
__device__ __forceinline__ void copy_tile_u(const seg_u& s, char* __restrict__ field,
                                            char* __restrict__ buf, uint32_t start, uint32_t end)
{
    using V = typename vec_t<W>::type;
    const uint32_t last = end - W;  // tiles hold whole rows: end - start is a multiple of W
    const uint32_t pol = s.fpol;
    for (uint32_t base = start + threadIdx.x * W; base < end; base += kU * kBlock * W)
    {
        uint32_t p[kU], idx[kU];
        int64_t extra[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) p[u] = min(base + uint32_t(u) * kBlock * W, last);
        V v[kU];
        if (!PACK)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u) v[u] = vload<V>(buf + p[u]);
        }
        if (s.mode == 0)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                const uint32_t row = fastdiv(p[u], s.mag_row);
                idx[u] = row;
                extra[u] = int64_t(p[u] - row * s.row_bytes);
            }
        }
        else if (s.mode == 1)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                const uint32_t row = fastdiv(p[u], s.mag_row);
                const uint32_t i = fastdiv(row, s.mag_inner);
                idx[u] = i;
                extra[u] = int64_t(row - i * s.row_levels) * s.level_stride_b +
                           int64_t(p[u] - row * s.row_bytes);
            }
        }
        else
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                const uint32_t row = fastdiv(p[u], s.mag_row);
                const uint32_t l = fastdiv(row, s.mag_inner);
                idx[u] = row - l * s.n;
                extra[u] = int64_t(l) * s.level_stride_b + int64_t(p[u] - row * s.row_bytes);
            }
        }
        int64_t lid[kU];
        if (s.lid64)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u) lid[u] = ((const GHX_GLOBAL int64_t*)(s.lids))[idx[u]];
        }
        else
        {
#pragma unroll
            for (int u = 0; u < kU; ++u) lid[u] = ((const GHX_GLOBAL int32_t*)(s.lids))[idx[u]];
        }
        int64_t fo[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) fo[u] = s.field_off + lid[u] * s.index_stride_b + extra[u];
        if (PACK)
        {
            if (pol & 1u)
            {
#pragma unroll
                for (int u = 0; u < kU; ++u) v[u] = fload<V>(field + fo[u], 1u);
            }
            else
            {
#pragma unroll
                for (int u = 0; u < kU; ++u) v[u] = vload<V>(field + fo[u]);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) vstore<V>(buf + p[u], v[u]);
        }
        else if (pol & 2u)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u) fstore<V>(field + fo[u], v[u], 2u);
        }
        else
        {
#pragma unroll
            for (int u = 0; u < kU; ++u) vstore<V>(field + fo[u], v[u]);
        }
    }
}

template<bool PACK, int UU>
__device__ __forceinline__ void copy_any(const seg_u& s, char* field, char* buf, uint32_t start,
                                         uint32_t end, int w)
{
    switch (w)
    {
        case 4: copy_tile_u<PACK, 16, UU>(s, field, buf, start, end); break;
        case 3: copy_tile_u<PACK, 8, UU>(s, field, buf, start, end); break;
        case 2: copy_tile_u<PACK, 4, UU>(s, field, buf, start, end); break;
        case 1: copy_tile_u<PACK, 2, UU>(s, field, buf, start, end); break;
        default: copy_tile_u<PACK, 1, UU>(s, field, buf, start, end); break;
    }
}

template<bool PACK, int UU, typename Seg>
__device__ __forceinline__ void copy_any(const Seg& s, char* field, char* buf, uint32_t start,
                                         uint32_t end, int w)
{
    if constexpr (!PACK)
        if (s.pipe && w == 4)  // long rows in tiles of several steps (planner: unpack_tile_bytes)
        {
            unpack_tile_pipelined<16>(s, field, buf, start, end);
            return;
        }
    if constexpr (std::is_same_v<Seg, seg_s>)
    {
        if (s.amode == 1)  // the short form for the widths fp32/fp64 fields give
        {
            switch (w)
            {
                case 4: copy_tile<PACK, 16, Seg, 1, UU>(s, field, buf, start, end); return;
                case 3: copy_tile<PACK, 8, Seg, 1, UU>(s, field, buf, start, end); return;
                case 2: copy_tile<PACK, 4, Seg, 1, UU>(s, field, buf, start, end); return;
                default: break;
            }
        }
        else if (s.amode == 2 && w == 4)
        {
            copy_tile<PACK, 16, Seg, 2, UU>(s, field, buf, start, end);
            return;
        }
    }
    switch (w)
    {
        case 4: copy_tile<PACK, 16>(s, field, buf, start, end); break;
        case 3: copy_tile<PACK, 8>(s, field, buf, start, end); break;
        case 2: copy_tile<PACK, 4>(s, field, buf, start, end); break;
        case 1: copy_tile<PACK, 2>(s, field, buf, start, end); break;
        default: copy_tile<PACK, 1>(s, field, buf, start, end); break;
    }
}

// RUNS (unstructured only): every segment of the plan takes the run path (copy_runs); the host
// (uplan::execute) launches this variant only when runs_ok holds for all of them, so the
// general path's registers do not weigh on it and vice versa.
// DBL (double-buffered buffers, the direct exchange's one-launch epochs): the launch uses, for
// every buffer slot with a second copy, the copy of this exchange's parity, read once per
// workgroup from the epoch counter in device memory (a captured graph alternates on replay).
__device__ __forceinline__ bool odd_parity(const kargs& a)
{
    return ((__hip_atomic_load(a.parity_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) +
             a.parity_add) & 1) != 0;
}

// REC (tile records, g_tune.tile_records): the workgroup's first load is its own record at
// tile_recs[blockIdx.x] (the segment, with the tile's index in first_tile), so the chain ahead
// of the first data load is one table load instead of tile table -> segment. The grid never
// exceeds n_tiles (grid_for_tiles), so the first tile needs no bound check either.
template<bool PACK, typename Seg, bool RUNS = false, bool DBL = false, int UU = kU, bool REC = false>
__global__ __launch_bounds__(kBlock) void k_copy(kargs a)
{
    const Seg* __restrict__ segs = static_cast<const Seg*>(REC ? a.tile_recs : a.segs);
    bool odd = false;
    if constexpr (DBL) odd = odd_parity(a);
    uint32_t t = blockIdx.x;
    do
    {
        Seg s;
        uint32_t ti;
        if constexpr (REC)
        {
            s = segs[t];
            ti = s.first_tile;
        }
        else
        {
            const uint32_t si = a.tile_seg[2 * t];
            ti = a.tile_seg[2 * t + 1];
            s = segs[si];
        }
        const uint32_t start = ti * s.tile_bytes;
        const uint32_t end = min(start + s.tile_bytes, s.bytes);
        char* field = reinterpret_cast<char*>(a.field_ptr[s.field_slot]);
        char* buf = reinterpret_cast<char*>(a.buf_ptr[s.buf_slot]) + s.buf_off;
        if constexpr (DBL)
            if (odd) buf += a.dbl_off[s.buf_slot];
        if constexpr (RUNS)
        {
            if (s.row_bytes == 8) copy_runs<PACK, 8>(s, field, buf, start, end);
            else copy_runs<PACK, 4>(s, field, buf, start, end);
        }
        else
        {
            int w = s.wlog2;
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(field)));
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(buf)));
            copy_any<PACK, UU>(s, field, buf, start, end, w);
        }
        t += gridDim.x;
    } while (t < a.n_tiles);
}

// Lane-local self tile with store-to-load forwarding: the unpack half needs exactly the buffer
// bytes this lane has just stored (same positions, same width), so it takes them from the
// registers instead of loading them back: field interior -> register -> buffer store AND halo
// store. Every buffer byte and every halo byte is still written; what disappears is the
// buffer read-back (which a lane-local read-back served from L2, or, for ~20 % of it, from HBM:
// TCC_EA0_RDREQ 573k against 461k for the field reads alone).
// AM: 0 general; 1 both segments in the short form with one division (copy_tile's AM 1).
template<int W, int AM = 0>
__device__ __forceinline__ void self_forward(const seg_s& s, const seg_s& q,
                                             char* __restrict__ fp, char* __restrict__ fu,
                                             char* __restrict__ buf, uint32_t start, uint32_t end)
{
    using V = typename vec_t<W>::type;
    using off_t = std::conditional_t<AM == 0, int64_t, uint32_t>;
    const uint32_t pol_p = s.fpol, pol_u = q.fpol;
    if constexpr (AM != 0)
    {
        fp += s.field_off;
        fu += q.field_off;
    }
    for (uint32_t base = start + threadIdx.x * W; base < end; base += kU * kBlock * W)
    {
        V v[kU];
        off_t op[kU], ou[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * W;
            if (p < end)
            {
                if constexpr (AM == 0)
                {
                    op[u] = field_offset_s(s, p);
                    ou[u] = field_offset_s(q, p);
                }
                else
                {
                    op[u] = field_offset_f<AM>(s, p);
                    ou[u] = field_offset_f<AM>(q, p);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * W;
            if (p < end) v[u] = fload<V>(fp + op[u], pol_p);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * W;
            if (p < end)
            {
                vstore<V>(buf + p, v[u]);
                fstore<V>(fu + ou[u], v[u], pol_u);
            }
        }
    }
}

// One tile of a fused self exchange (k_self, k_self_cs): pack segment s and unpack segment q
// cover the same buffer bytes with the same tiling. When both halves of the tile use the same
// vector width (always, for aligned fields) every lane unpacks exactly the bytes it packed:
// it writes the halo from the registers it stored the buffer from (self_forward), no barrier.
// Otherwise the workgroup packs its tile (field interior -> buffer), passes a workgroup barrier
// (its own stores are visible to its own waves), then unpacks the same bytes (buffer -> halo).
// PEERS: q.bytes == 0 marks a peer message of a mixed exchange (ghx_exchange_pack_self), which
// is packed only.
template<bool PEERS>
__device__ __forceinline__ void self_pair_tile(const seg_s& s, const seg_s& q, uint32_t ti,
                                               char* field_p, char* field_u, char* buf)
{
    const uint32_t start = ti * s.tile_bytes;
    const uint32_t end = min(start + s.tile_bytes, s.bytes);
    int wp = min(int(s.wlog2), ptr_wlog2(reinterpret_cast<uint64_t>(field_p)));
    wp = min(wp, ptr_wlog2(reinterpret_cast<uint64_t>(buf)));
    int wu = min(int(q.wlog2), ptr_wlog2(reinterpret_cast<uint64_t>(field_u)));
    wu = min(wu, ptr_wlog2(reinterpret_cast<uint64_t>(buf)));
    if constexpr (PEERS)
        if (q.bytes == 0)
        {
            copy_any<true, kU>(s, field_p, buf, start, end, wp);
            return;
        }
    if (wp == wu && s.amode == 1 && q.amode == 1 && wp >= 3)
    {
        if (wp == 4) self_forward<16, 1>(s, q, field_p, field_u, buf, start, end);
        else self_forward<8, 1>(s, q, field_p, field_u, buf, start, end);
        return;
    }
    if (wp == wu)
    {
        switch (wp)
        {
            case 4: self_forward<16>(s, q, field_p, field_u, buf, start, end); break;
            case 3: self_forward<8>(s, q, field_p, field_u, buf, start, end); break;
            case 2: self_forward<4>(s, q, field_p, field_u, buf, start, end); break;
            case 1: self_forward<2>(s, q, field_p, field_u, buf, start, end); break;
            default: self_forward<1>(s, q, field_p, field_u, buf, start, end); break;
        }
        return;
    }
    copy_any<true, kU>(s, field_p, buf, start, end, wp);
    __syncthreads();  // workgroup release/acquire: the tile's buffer bytes are complete
    copy_any<false, kU>(q, field_u, buf, start, end, wu);
    __syncthreads();  // the next tile of a grid-stride loop reuses the lanes
}

// Fused self exchange: every message is a self message (or, mixed, a peer message to pack).
// REC: pair records (upload_pair_records) — the workgroup loads its tile's pack and unpack
// segments side by side at tile_recs[2 * blockIdx.x], no tile-table load ahead of them.
template<bool DBL = false, bool REC = false>
__global__ __launch_bounds__(kBlock) void k_self(kargs a)
{
    const seg_s* __restrict__ ps = static_cast<const seg_s*>(a.segs);
    const seg_s* __restrict__ us = static_cast<const seg_s*>(a.segs2);
    const seg_s* __restrict__ rec = static_cast<const seg_s*>(a.tile_recs);
    bool odd = false;
    if constexpr (DBL) odd = odd_parity(a);
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        seg_s s, q;
        uint32_t ti;
        if constexpr (REC)
        {
            s = rec[2 * t];
            q = rec[2 * t + 1];
            ti = s.first_tile;
        }
        else
        {
            const uint32_t si = a.tile_seg[2 * t];
            ti = a.tile_seg[2 * t + 1];
            s = ps[si];
            q = us[si];
        }
        char* field_p = reinterpret_cast<char*>(a.field_ptr[s.field_slot]);
        char* field_u = reinterpret_cast<char*>(a.field_ptr[q.field_slot]);
        char* buf = reinterpret_cast<char*>(a.buf_ptr[s.buf_slot]) + s.buf_off;
        if constexpr (DBL)
            if (odd) buf += a.dbl_off[s.buf_slot];
        self_pair_tile<true>(s, q, ti, field_p, field_u, buf);
    }
}

// Zero-copy put: element p of the virtual message is read from the source field through the
// pack segment's addressing and written to the target field (peer memory or local) through the
// unpack segment's addressing, register to register — no buffer.
template<int W, int AM = 0>
__device__ __forceinline__ void copy_direct(const seg_s& s, const seg_s& q,
                                            const char* __restrict__ src, char* __restrict__ dst,
                                            uint32_t start, uint32_t end)
{
    using V = typename vec_t<W>::type;
    using off_t = std::conditional_t<AM == 0, int64_t, uint32_t>;
    if constexpr (AM != 0)
    {
        src += s.field_off;
        dst += q.field_off;
    }
    for (uint32_t base = start + threadIdx.x * W; base < end; base += kU * kBlock * W)
    {
        V v[kU];
        off_t fd[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * W;
            if (p < end)
            {
                if constexpr (AM == 0)
                {
                    v[u] = vload<V>(src + field_offset_s(s, p));
                    fd[u] = field_offset_s(q, p);
                }
                else
                {
                    v[u] = vload<V>(src + field_offset_f<AM>(s, p));
                    fd[u] = field_offset_f<AM>(q, p);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * W;
            if (p < end) vstore<V>(dst + fd[u], v[u]);
        }
    }
}

// One tile of a put (k_put, k_put_cs) at the widest vector both segments and both pointers allow.
__device__ __forceinline__ void put_pair_tile(const seg_s& s, const seg_s& q, uint32_t ti,
                                              const char* src, char* dst)
{
    const uint32_t start = ti * s.tile_bytes;
    const uint32_t end = min(start + s.tile_bytes, s.bytes);
    int w = min(int(s.wlog2), int(q.wlog2));
    w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(src)));
    w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(dst)));
    if (s.amode == 1 && q.amode == 1 && w >= 3)
    {
        if (w == 4) copy_direct<16, 1>(s, q, src, dst, start, end);
        else copy_direct<8, 1>(s, q, src, dst, start, end);
        return;
    }
    switch (w)
    {
        case 4: copy_direct<16>(s, q, src, dst, start, end); break;
        case 3: copy_direct<8>(s, q, src, dst, start, end); break;
        case 2: copy_direct<4>(s, q, src, dst, start, end); break;
        case 1: copy_direct<2>(s, q, src, dst, start, end); break;
        default: copy_direct<1>(s, q, src, dst, start, end); break;
    }
}

template<bool REC = false>
__global__ __launch_bounds__(kBlock) void k_put(kargs a)
{
    const seg_s* __restrict__ ps = static_cast<const seg_s*>(a.segs);
    const seg_s* __restrict__ qs = static_cast<const seg_s*>(a.segs2);
    const seg_s* __restrict__ rec = static_cast<const seg_s*>(a.tile_recs);
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        seg_s s, q;
        uint32_t ti;
        if constexpr (REC)
        {
            s = rec[2 * t];
            q = rec[2 * t + 1];
            ti = s.first_tile;
        }
        else
        {
            const uint32_t si = a.tile_seg[2 * t];
            ti = a.tile_seg[2 * t + 1];
            s = ps[si];
            q = qs[si];
        }
        put_pair_tile(s, q, ti, reinterpret_cast<const char*>(a.field_ptr[s.field_slot]),
                      reinterpret_cast<char*>(a.buf_ptr[q.field_slot]));
    }
}

// An element of 2^E bytes: element-wide when `aligned`, else byte by byte (a buffer or field
// whose base or strides are not multiples of the element size).
template<int E>
__device__ __forceinline__ typename vec_t<(1 << E)>::type load_elem(const char* p, bool aligned)
{
    using V = typename vec_t<(1 << E)>::type;
    if (aligned) return vload<V>(p);
    unsigned char b[1 << E];
#pragma unroll
    for (int k = 0; k < (1 << E); ++k) b[k] = vload<unsigned char>(p + k);
    V v;
    __builtin_memcpy(&v, b, sizeof(V));
    return v;
}

template<int E>
__device__ __forceinline__ void store_elem(char* p, typename vec_t<(1 << E)>::type v, bool aligned)
{
    using V = typename vec_t<(1 << E)>::type;
    if (aligned)
    {
        vstore<V>(p, v);
        return;
    }
    unsigned char b[1 << E];
    __builtin_memcpy(b, &v, sizeof(V));
#pragma unroll
    for (int k = 0; k < (1 << E); ++k) vstore<unsigned char>(p + k, b[k]);
}

// Negation of a vector component (cubed_sphere/field_descriptor.hpp:97-104): sign-bit flip
// (kind 1) or two's-complement negate (2) of a 4- or 8-byte element; other widths are opaque.
template<int E>
__device__ __forceinline__ typename vec_t<(1 << E)>::type negate_elem(
    typename vec_t<(1 << E)>::type v, uint32_t kind)
{
    if constexpr (E == 2)
        v = kind == 1 ? (v ^ 0x80000000u) : (0u - v);
    else if constexpr (E == 3)
    {
        if (kind == 1) v.y ^= 0x80000000u;
        else
        {
            const uint64_t w = 0ull - ((uint64_t(v.y) << 32) | v.x);
            v.x = uint32_t(w);
            v.y = uint32_t(w >> 32);
        }
    }
    return v;
}

// The transformed tile walk (cubed sphere) of k_unpack_x, k_self_cs and k_put_cs:
// one workgroup per tile record, one element per lane.
//
// The tile is a sub-box of the message's dense box (the halo in the neighbour tile's
// coordinates), walked in FIELD order: the record's axes are sorted by ascending |stride| of the
// RECEIVING field, so consecutive lanes write consecutive field elements of one run and a wave's
// store covers whole runs (the side that may cross xGMI in a put), while its loads fall on a few
// long pieces of buffer rows or of the sending field's rows (for an x-stride-1 field and a halo
// of width H rotated by 90 degrees: H rows of up to 256 / H elements each, written as H-element
// field runs, where the element-row form of the ordinary kernel issues one store per line). A
// reversed axis is a negative stride. Vector components are negated in registers between the
// load and the store to the field. No LDS: staging the tile through LDS (buffer range read
// lane-linear, transposed reads from LDS) measured slower at every tile size: the launch is
// latency-bound and the LDS round trip and its barrier sit in the dependent chain. No barrier
// and no ordering among workgroups either: the planner has checked that no cell a launch reads
// is a cell it writes (it refuses source boxes that reach into the sender's halo). Plain global
// stores only: the destination may be a peer's mapped memory, and the epochs' system-scope
// release at close covers nothing else.
// FROM_FIELD: the element comes from the sending field (r->src_*), not from its buffer cell.
// TO_CELL: it is also stored, as loaded, to its buffer cell.
template<int E, bool FROM_FIELD, bool TO_CELL>
__device__ __forceinline__ void walk_x_tile(const seg_x& s, const seg_xs* r,
                                            const char* __restrict__ send, char* __restrict__ cells,
                                            char* __restrict__ field, bool aligned)
{
    const uint32_t total = s.tdim[0] * s.tdim[1] * s.tdim[2] * s.tdim[3];
    for (uint32_t i = threadIdx.x; i < total; i += kBlock)
    {
        uint32_t c[4];
        if (!tile_decode(s, i, c)) continue;
        char* cell = nullptr;
        if constexpr (!FROM_FIELD || TO_CELL) cell = cells + (size_t(tile_cell(s, c)) << E);
        const char* from = cell;
        if constexpr (FROM_FIELD) from = affine_offset(send + r->src_off, r->src_stride, c);
        const auto v = load_elem<E>(from, aligned);
        auto w = v;
        if (s.neg_mask)  // uniform per tile: most tiles negate nothing
        {
            if (tile_negates(s, c)) w = negate_elem<E>(v, s.neg_kind);
        }
        // both stores after the negation: nothing then waits between them for the first to land
        if constexpr (TO_CELL) store_elem<E>(cell, v, aligned);
        store_elem<E>(affine_offset(field + s.field_off, s.stride, c), w, aligned);
    }
}

// The walk at the record's element width. Element-wide accesses when the source, the buffer
// (where the form uses it), the destination and every stride used are element-aligned (uniform
// per tile; a mapped peer pointer's alignment is a run-time fact).
template<bool FROM_FIELD, bool TO_CELL>
__device__ __forceinline__ void walk_x(const seg_x& s, const seg_xs* r, const char* send,
                                       char* cells, char* field)
{
    const uint64_t em = (1u << s.elog2) - 1u;
    uint64_t strides = uint64_t(s.stride[0]) | uint64_t(s.stride[1]) | uint64_t(s.stride[2]) |
                       uint64_t(s.stride[3]);
    bool aligned = true;
    if constexpr (FROM_FIELD)
    {
        aligned = ((reinterpret_cast<uint64_t>(send) + uint64_t(r->src_off)) & em) == 0;
        strides |= uint64_t(r->src_stride[0]) | uint64_t(r->src_stride[1]) |
                   uint64_t(r->src_stride[2]) | uint64_t(r->src_stride[3]);
    }
    if constexpr (!FROM_FIELD || TO_CELL) aligned = aligned && (reinterpret_cast<uint64_t>(cells) & em) == 0;
    aligned = aligned && ((reinterpret_cast<uint64_t>(field) + uint64_t(s.field_off)) & em) == 0 &&
              (strides & em) == 0;
    switch (s.elog2)
    {
        case 4: walk_x_tile<4, FROM_FIELD, TO_CELL>(s, r, send, cells, field, aligned); break;
        case 3: walk_x_tile<3, FROM_FIELD, TO_CELL>(s, r, send, cells, field, aligned); break;
        case 2: walk_x_tile<2, FROM_FIELD, TO_CELL>(s, r, send, cells, field, aligned); break;
        case 1: walk_x_tile<1, FROM_FIELD, TO_CELL>(s, r, send, cells, field, aligned); break;
        default: walk_x_tile<0, FROM_FIELD, TO_CELL>(s, r, send, cells, field, aligned); break;
    }
}

// Transformed unpack: buffer cell -> receiving field, one workgroup per seg_x record.
__global__ __launch_bounds__(kBlock) void k_unpack_x(kargs a)
{
    const seg_x* __restrict__ recs = static_cast<const seg_x*>(a.tile_recs);
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        const seg_x s = recs[t];
        walk_x<false, false>(s, nullptr, nullptr,
                             reinterpret_cast<char*>(a.buf_ptr[s.buf_slot]) + s.buf_off,
                             reinterpret_cast<char*>(a.field_ptr[s.field_slot]));
    }
}

// The transpose of walk_x_tile<E, false, false> (the reverse pack of the cubed-sphere adjoint,
// DESIGN.md §4.8): the same tile record, decode and offsets with the data direction reversed —
// each lane loads its element of the receiving field, negates it where the transform does (the
// sign matrix is diagonal: its transpose is itself) and stores it to its buffer cell. The tile is
// still walked in field order, so a wave's loads cover whole field runs and its stores fall on a
// few pieces of buffer rows. A sibling and not a flag of walk_x_tile: the three forward kernels
// keep their code as it is.
template<int E>
__device__ __forceinline__ void pack_x_tile(const seg_x& s, const char* __restrict__ field,
                                            char* __restrict__ cells, bool aligned)
{
    const uint32_t total = s.tdim[0] * s.tdim[1] * s.tdim[2] * s.tdim[3];
    for (uint32_t i = threadIdx.x; i < total; i += kBlock)
    {
        uint32_t c[4];
        if (!tile_decode(s, i, c)) continue;
        auto v = load_elem<E>(affine_offset(field + s.field_off, s.stride, c), aligned);
        if (s.neg_mask)  // uniform per tile: most tiles negate nothing
        {
            if (tile_negates(s, c)) v = negate_elem<E>(v, s.neg_kind);
        }
        store_elem<E>(cells + (size_t(tile_cell(s, c)) << E), v, aligned);
    }
}

// Element-wide accesses when the field, the buffer and every field stride are element-aligned
// (uniform per tile), as in walk_x.
__device__ __forceinline__ void pack_x(const seg_x& s, const char* field, char* cells)
{
    const uint64_t em = (1u << s.elog2) - 1u;
    const uint64_t strides = uint64_t(s.stride[0]) | uint64_t(s.stride[1]) | uint64_t(s.stride[2]) |
                             uint64_t(s.stride[3]);
    const bool aligned = (reinterpret_cast<uint64_t>(cells) & em) == 0 &&
                         ((reinterpret_cast<uint64_t>(field) + uint64_t(s.field_off)) & em) == 0 &&
                         (strides & em) == 0;
    switch (s.elog2)
    {
        case 4: pack_x_tile<4>(s, field, cells, aligned); break;
        case 3: pack_x_tile<3>(s, field, cells, aligned); break;
        case 2: pack_x_tile<2>(s, field, cells, aligned); break;
        case 1: pack_x_tile<1>(s, field, cells, aligned); break;
        default: pack_x_tile<0>(s, field, cells, aligned); break;
    }
}

// Transformed reverse pack: receiving field -> buffer cell, over k_unpack_x's own records.
__global__ __launch_bounds__(kBlock) void k_pack_x(kargs a)
{
    const seg_x* __restrict__ recs = static_cast<const seg_x*>(a.tile_recs);
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        const seg_x s = recs[t];
        pack_x(s, reinterpret_cast<const char*>(a.field_ptr[s.field_slot]),
               reinterpret_cast<char*>(a.buf_ptr[s.buf_slot]) + s.buf_off);
    }
}

// Fused cubed-sphere self exchange: pack and rotating unpack of an exchange whose every message
// stays on this device, in ONE launch. Blocks [0, n_pair_tiles) take a pair record as k_self's
// record form does (spaces whose pack and unpack segments cover the same bytes with the same
// rows); the blocks after them take a self tile record (seg_xs): sending field -> buffer cell
// (the send buffers hold the packed message afterwards) and receiving field, no buffer read-back.
__global__ __launch_bounds__(kBlock) void k_self_cs(kargs_cs a)
{
    const seg_s* __restrict__ pairs = static_cast<const seg_s*>(a.pair_recs);
    const seg_xs* __restrict__ xrecs = static_cast<const seg_xs*>(a.x_recs);
    const uint32_t n_tiles = a.n_pair_tiles + a.n_x_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x)
    {
        if (t < a.n_pair_tiles)  // uniform per workgroup
        {
            const seg_s s = pairs[2 * t];
            const seg_s q = pairs[2 * t + 1];
            self_pair_tile<false>(s, q, s.first_tile, reinterpret_cast<char*>(a.ptr[s.field_slot]),
                                  reinterpret_cast<char*>(a.ptr[q.field_slot]),
                                  reinterpret_cast<char*>(a.ptr[a.buf_base + s.buf_slot]) + s.buf_off);
            continue;
        }
        const seg_xs r = xrecs[t - a.n_pair_tiles];
        walk_x<true, true>(r.x, &r, reinterpret_cast<const char*>(a.ptr[r.src_slot]),
                           reinterpret_cast<char*>(a.ptr[a.buf_base + r.x.buf_slot]) + r.x.buf_off,
                           reinterpret_cast<char*>(a.ptr[r.x.field_slot]));
    }
}

// Cubed-sphere put: k_self_cs's walk without the buffer, the destination being any mapped field
// (this device's or a node-local peer's through IPC). Blocks [0, n_pair_tiles) take a pair record
// as k_put's record form does; the blocks after them take a put tile record (seg_xs, buffer side
// unused): sending field -> receiving field — 2 bytes of traffic per message byte against
// k_self_cs's 3.
__global__ __launch_bounds__(kBlock) void k_put_cs(kargs_pcs a)
{
    const seg_s* __restrict__ pairs = static_cast<const seg_s*>(a.pair_recs);
    const seg_xs* __restrict__ xrecs = static_cast<const seg_xs*>(a.x_recs);
    const uint32_t n_tiles = a.n_pair_tiles + a.n_x_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x)
    {
        if (t < a.n_pair_tiles)  // uniform per workgroup
        {
            const seg_s s = pairs[2 * t];
            const seg_s q = pairs[2 * t + 1];
            put_pair_tile(s, q, s.first_tile, reinterpret_cast<const char*>(a.src_ptr[s.field_slot]),
                          reinterpret_cast<char*>(a.dst_ptr[q.field_slot]));
            continue;
        }
        const seg_xs r = xrecs[t - a.n_pair_tiles];
        walk_x<true, false>(r.x, &r, reinterpret_cast<const char*>(a.src_ptr[r.src_slot]), nullptr,
                            reinterpret_cast<char*>(a.dst_ptr[r.x.field_slot]));
    }
}

// ---------------------------------------------------------------------------------------------
// Index-list put (seg_up): send list on the sending field -> receive list on the receiving field.
// ---------------------------------------------------------------------------------------------

// kU lids of one table at idx[], all loads issued together (WIDE: int64 entries)
template<bool WIDE>
__device__ __forceinline__ void gather_lids(const void* table, const uint32_t (&idx)[kU], int64_t (&lid)[kU])
{
#pragma unroll
    for (int u = 0; u < kU; ++u)
    {
        if constexpr (WIDE) lid[u] = ((const GHX_GLOBAL int64_t*)(table))[idx[u]];
        else lid[u] = ((const GHX_GLOBAL int32_t*)(table))[idx[u]];
    }
}

// General path, the shape of copy_tile_u: per loop trip a lane takes kU message positions (one past
// the tile's end is clamped to the tile's last vector and moves the same bytes to the same
// address again), decodes each once into (index, level, remainder) by the common mode, then
// issues all kU index loads of the source table and all kU of the target table, all kU value
// loads from the source field, all kU stores to the target field. The uniform choices (table
// widths S64 / D64, vector width W: template arguments; the mode: one branch around the whole
// decode) stay out of the per-vector code, so no load waits for the one before it.
template<int W, bool S64, bool D64>
__device__ __forceinline__ void put_tile_u(const seg_up& s, const char* __restrict__ src,
                                           char* __restrict__ dst, uint32_t start, uint32_t end)
{
    using V = typename vec_t<W>::type;
    const uint32_t last = end - W;  // tiles hold whole rows: end - start is a multiple of W
    src += s.src_field_off;
    dst += s.dst_field_off;
    for (uint32_t base = start + threadIdx.x * W; base < end; base += kU * kBlock * W)
    {
        uint32_t idx[kU], lev[kU], rem[kU];
        if (s.mode == 0)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                const uint32_t p = min(base + uint32_t(u) * kBlock * W, last);
                idx[u] = fastdiv(p, s.mag_row);
                lev[u] = 0;
                rem[u] = p - idx[u] * s.row_bytes;
            }
        }
        else if (s.mode == 1)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                const uint32_t p = min(base + uint32_t(u) * kBlock * W, last);
                const uint32_t row = fastdiv(p, s.mag_row);
                idx[u] = fastdiv(row, s.mag_inner);
                lev[u] = row - idx[u] * s.row_levels;
                rem[u] = p - row * s.row_bytes;
            }
        }
        else
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                const uint32_t p = min(base + uint32_t(u) * kBlock * W, last);
                const uint32_t row = fastdiv(p, s.mag_row);
                lev[u] = fastdiv(row, s.mag_inner);
                idx[u] = row - lev[u] * s.n;
                rem[u] = p - row * s.row_bytes;
            }
        }
        int64_t sl[kU], dl[kU];
        gather_lids<S64>(s.src_lids, idx, sl);
        gather_lids<D64>(s.dst_lids, idx, dl);
        V v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)
            v[u] = vload<V>(src + sl[u] * s.src_index_stride_b + int64_t(lev[u]) * s.src_level_stride_b + rem[u]);
#pragma unroll
        for (int u = 0; u < kU; ++u)
            vstore<V>(dst + dl[u] * s.dst_index_stride_b + int64_t(lev[u]) * s.dst_level_stride_b + rem[u], v[u]);
    }
}

template<bool S64, bool D64>
__device__ __forceinline__ void put_tile_u_w(const seg_up& s, const char* src, char* dst,
                                             uint32_t start, uint32_t end, int w)
{
    switch (w)
    {
        case 4: put_tile_u<16, S64, D64>(s, src, dst, start, end); break;
        case 3: put_tile_u<8, S64, D64>(s, src, dst, start, end); break;
        case 2: put_tile_u<4, S64, D64>(s, src, dst, start, end); break;
        case 1: put_tile_u<2, S64, D64>(s, src, dst, start, end); break;
        default: put_tile_u<1, S64, D64>(s, src, dst, start, end); break;
    }
}

// K consecutive lids of one table from position r0 with one vector load per 16 B (r0 a multiple
// of K: the table and the tile start are 16-B aligned, a lane's chunk K rows)
template<int K>
__device__ __forceinline__ void load_lid_chunk(const void* table, bool wide, uint32_t r0, int64_t (&l)[K])
{
    if (wide)
    {
        const GHX_GLOBAL vec_t<16>::type* p = (const GHX_GLOBAL vec_t<16>::type*)((const int64_t*)(table) + r0);
#pragma unroll
        for (int j = 0; j < K; j += 2)
        {
            const auto q = p[j / 2];
            l[j] = int64_t(uint64_t(q.x) | (uint64_t(q.y) << 32));
            l[j + 1] = int64_t(uint64_t(q.z) | (uint64_t(q.w) << 32));
        }
    }
    else if constexpr (K == 2)
    {
        const auto q = *(const GHX_GLOBAL vec_t<8>::type*)((const int32_t*)(table) + r0);
        l[0] = int32_t(q.x);
        l[1] = int32_t(q.y);
    }
    else
    {
        const auto q = *(const GHX_GLOBAL vec_t<16>::type*)((const int32_t*)(table) + r0);
        l[0] = int32_t(q.x);
        l[1] = int32_t(q.y);
        l[2] = int32_t(q.z);
        l[3] = int32_t(q.w);
    }
}

__device__ __forceinline__ int64_t load_lid_one(const void* table, bool wide, uint32_t i)
{
    if (wide) return ((const GHX_GLOBAL int64_t*)(table))[i];
    return ((const GHX_GLOBAL int32_t*)(table))[i];
}

// Run path, the shape of copy_runs: rows of L = 4 or 8 bytes (mode 0), a lane owns K = 16 / L
// consecutive message rows and loads its K lids of each table with one vector load. A side whose
// K lids form a run (lid[j] = lid[0] + j) and whose rows of consecutive lids are adjacent in its
// field (seg_up::src_runs / dst_runs: its index stride is L) moves the 16 bytes in ONE access,
// else row by row; the two sides decide independently, so a wave may hold all four combinations
// (masked). A side that never forms runs still takes its offsets from its own index stride. A
// segment tail of fewer than K rows goes row by row; no lid is read at or beyond n.
template<int L>
__device__ __forceinline__ void put_runs(const seg_up& s, const char* __restrict__ src,
                                         char* __restrict__ dst, uint32_t start, uint32_t end)
{
    using V = typename vec_t<16>::type;
    using R = typename vec_t<L>::type;
    constexpr int K = 16 / L;
    src += s.src_field_off;
    dst += s.dst_field_off;
    for (uint32_t base = start + threadIdx.x * 16; base < end; base += kU * kBlock * 16)
    {
        int64_t so[kU][K], to[kU][K];
        uint32_t full = 0, srun = 0, drun = 0;  // bit u: chunk u holds K rows / its side is a run
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * 16;
            if (p >= end) continue;
            const uint32_t r0 = p / L;
            int64_t ls[K], ld[K];
            if (p + 16 <= end)
            {
                full |= 1u << u;
                load_lid_chunk<K>(s.src_lids, s.src_lid64, r0, ls);
                load_lid_chunk<K>(s.dst_lids, s.dst_lid64, r0, ld);
                bool cs = s.src_runs != 0, cd = s.dst_runs != 0;
#pragma unroll
                for (int j = 1; j < K; ++j)
                {
                    cs = cs && ls[j] == ls[0] + j;
                    cd = cd && ld[j] == ld[0] + j;
                }
                if (cs) srun |= 1u << u;
                if (cd) drun |= 1u << u;
            }
            else
            {
#pragma unroll
                for (int j = 0; j < K; ++j)
                {
                    const bool in = p + j * L < end;
                    ls[j] = in ? load_lid_one(s.src_lids, s.src_lid64, r0 + j) : 0;
                    ld[j] = in ? load_lid_one(s.dst_lids, s.dst_lid64, r0 + j) : 0;
                }
            }
#pragma unroll
            for (int j = 0; j < K; ++j)
            {
                so[u][j] = ls[j] * s.src_index_stride_b;
                to[u][j] = ld[j] * s.dst_index_stride_b;
            }
        }
        V v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            if (!(full >> u & 1u)) continue;
            if (srun >> u & 1u)
            {
                const v4_a4 x = vload<v4_a4>(src + so[u][0]);
                v[u] = V{x.x, x.y, x.z, x.w};
            }
            else
            {
                R w[K];
#pragma unroll
                for (int j = 0; j < K; ++j) w[j] = vload<R>(src + so[u][j]);
                v[u] = assemble<L>(w);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * 16;
            if (p >= end) continue;
            if (!(full >> u & 1u))
            {
                // segment tail: fewer than K rows left, row by row
#pragma unroll
                for (int j = 0; j < K; ++j)
                {
                    if (p + j * L >= end) break;
                    vstore<R>(dst + to[u][j], vload<R>(src + so[u][j]));
                }
                continue;
            }
            if (drun >> u & 1u)
                vstore<v4_a4>(dst + to[u][0], v4_a4{v[u].x, v[u].y, v[u].z, v[u].w});
            else
            {
                R w[K];
                split<L>(v[u], w);
#pragma unroll
                for (int j = 0; j < K; ++j) vstore<R>(dst + to[u][j], w[j]);
            }
        }
    }
}

// One tile record per workgroup at its block index (grid-stride beyond the grid cap). RUNS: every
// segment of the plan takes the run path (uput_plan::execute decides with the launch's pointers),
// so neither path's registers weigh on the other. Source field slot s at field_ptr[s], target
// field slot d at buf_ptr[d], as k_put's.
template<bool RUNS>
__global__ __launch_bounds__(kBlock) void k_put_u(kargs a)
{
    const seg_up* __restrict__ recs = static_cast<const seg_up*>(a.tile_recs);
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        const seg_up s = recs[t];
        const uint32_t start = s.first_tile * s.tile_bytes;
        const uint32_t end = min(start + s.tile_bytes, s.bytes);
        const char* src = reinterpret_cast<const char*>(a.field_ptr[s.src_slot]);
        char* dst = reinterpret_cast<char*>(a.buf_ptr[s.dst_slot]);
        if constexpr (RUNS)
        {
            if (s.row_bytes == 8) put_runs<8>(s, src, dst, start, end);
            else put_runs<4>(s, src, dst, start, end);
        }
        else
        {
            int w = s.wlog2;
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(src)));
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(dst)));
            if (s.src_lid64)
            {
                if (s.dst_lid64) put_tile_u_w<true, true>(s, src, dst, start, end, w);
                else put_tile_u_w<true, false>(s, src, dst, start, end, w);
            }
            else if (s.dst_lid64) put_tile_u_w<false, true>(s, src, dst, start, end, w);
            else put_tile_u_w<false, false>(s, src, dst, start, end, w);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Fused index-list self exchange (seg_up with its buffer side): send list on the sending field ->
// the send buffer AND the receive list on the receiving field, no buffer byte read.
// ---------------------------------------------------------------------------------------------

// General path, the shape of put_tile_u: per loop trip a lane decodes its kU message positions
// once, issues the kU index loads of the source table and the kU of the target table together,
// then the kU value loads, the kU buffer stores (message position p at buf + p: consecutive lanes
// at consecutive addresses, the coalesced side) and the kU target stores. A position past the
// tile's end is clamped to the tile's last vector and moves the same bytes to the same two
// addresses again. `buf` points at the segment's first message row.
template<int W, bool S64, bool D64>
__device__ __forceinline__ void self_tile_u(const seg_up& s, const char* __restrict__ src,
                                            char* __restrict__ dst, char* __restrict__ buf,
                                            uint32_t start, uint32_t end)
{
    using V = typename vec_t<W>::type;
    const uint32_t last = end - W;  // tiles hold whole rows: end - start is a multiple of W
    src += s.src_field_off;
    dst += s.dst_field_off;
    for (uint32_t base = start + threadIdx.x * W; base < end; base += kU * kBlock * W)
    {
        uint32_t pos[kU], idx[kU], lev[kU], rem[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) pos[u] = min(base + uint32_t(u) * kBlock * W, last);
        if (s.mode == 0)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                idx[u] = fastdiv(pos[u], s.mag_row);
                lev[u] = 0;
                rem[u] = pos[u] - idx[u] * s.row_bytes;
            }
        }
        else if (s.mode == 1)
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                const uint32_t row = fastdiv(pos[u], s.mag_row);
                idx[u] = fastdiv(row, s.mag_inner);
                lev[u] = row - idx[u] * s.row_levels;
                rem[u] = pos[u] - row * s.row_bytes;
            }
        }
        else
        {
#pragma unroll
            for (int u = 0; u < kU; ++u)
            {
                const uint32_t row = fastdiv(pos[u], s.mag_row);
                lev[u] = fastdiv(row, s.mag_inner);
                idx[u] = row - lev[u] * s.n;
                rem[u] = pos[u] - row * s.row_bytes;
            }
        }
        int64_t sl[kU], dl[kU];
        gather_lids<S64>(s.src_lids, idx, sl);
        gather_lids<D64>(s.dst_lids, idx, dl);
        V v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)
            v[u] = vload<V>(src + sl[u] * s.src_index_stride_b + int64_t(lev[u]) * s.src_level_stride_b + rem[u]);
#pragma unroll
        for (int u = 0; u < kU; ++u) vstore<V>(buf + pos[u], v[u]);
#pragma unroll
        for (int u = 0; u < kU; ++u)
            vstore<V>(dst + dl[u] * s.dst_index_stride_b + int64_t(lev[u]) * s.dst_level_stride_b + rem[u], v[u]);
    }
}

template<bool S64, bool D64>
__device__ __forceinline__ void self_tile_u_w(const seg_up& s, const char* src, char* dst, char* buf,
                                              uint32_t start, uint32_t end, int w)
{
    switch (w)
    {
        case 4: self_tile_u<16, S64, D64>(s, src, dst, buf, start, end); break;
        case 3: self_tile_u<8, S64, D64>(s, src, dst, buf, start, end); break;
        case 2: self_tile_u<4, S64, D64>(s, src, dst, buf, start, end); break;
        case 1: self_tile_u<2, S64, D64>(s, src, dst, buf, start, end); break;
        default: self_tile_u<1, S64, D64>(s, src, dst, buf, start, end); break;
    }
}

// Run path, the shape of put_runs: rows of L = 4 or 8 bytes (mode 0), a lane owns a 16-byte
// message chunk (K = 16 / L rows) and loads its K lids of each table with one vector load. Each
// field side decides on its own whether its chunk is ONE 16-byte access (its K lids a run, its
// rows adjacent) or K row accesses; the buffer side is always ONE 16-byte store at buf + p (the
// launch takes this path only where every chunk of the buffer is 16-B aligned). A segment tail
// of fewer than K rows goes row by row on all three sides; no lid is read at or beyond n.
template<int L>
__device__ __forceinline__ void self_runs(const seg_up& s, const char* __restrict__ src,
                                          char* __restrict__ dst, char* __restrict__ buf,
                                          uint32_t start, uint32_t end)
{
    using V = typename vec_t<16>::type;
    using R = typename vec_t<L>::type;
    constexpr int K = 16 / L;
    src += s.src_field_off;
    dst += s.dst_field_off;
    for (uint32_t base = start + threadIdx.x * 16; base < end; base += kU * kBlock * 16)
    {
        int64_t so[kU][K], to[kU][K];
        uint32_t full = 0, srun = 0, drun = 0;  // bit u: chunk u holds K rows / its side is a run
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * 16;
            if (p >= end) continue;
            const uint32_t r0 = p / L;
            int64_t ls[K], ld[K];
            if (p + 16 <= end)
            {
                full |= 1u << u;
                load_lid_chunk<K>(s.src_lids, s.src_lid64, r0, ls);
                load_lid_chunk<K>(s.dst_lids, s.dst_lid64, r0, ld);
                bool cs = s.src_runs != 0, cd = s.dst_runs != 0;
#pragma unroll
                for (int j = 1; j < K; ++j)
                {
                    cs = cs && ls[j] == ls[0] + j;
                    cd = cd && ld[j] == ld[0] + j;
                }
                if (cs) srun |= 1u << u;
                if (cd) drun |= 1u << u;
            }
            else
            {
#pragma unroll
                for (int j = 0; j < K; ++j)
                {
                    const bool in = p + j * L < end;
                    ls[j] = in ? load_lid_one(s.src_lids, s.src_lid64, r0 + j) : 0;
                    ld[j] = in ? load_lid_one(s.dst_lids, s.dst_lid64, r0 + j) : 0;
                }
            }
#pragma unroll
            for (int j = 0; j < K; ++j)
            {
                so[u][j] = ls[j] * s.src_index_stride_b;
                to[u][j] = ld[j] * s.dst_index_stride_b;
            }
        }
        V v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            if (!(full >> u & 1u)) continue;
            if (srun >> u & 1u)
            {
                const v4_a4 x = vload<v4_a4>(src + so[u][0]);
                v[u] = V{x.x, x.y, x.z, x.w};
            }
            else
            {
                R w[K];
#pragma unroll
                for (int j = 0; j < K; ++j) w[j] = vload<R>(src + so[u][j]);
                v[u] = assemble<L>(w);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (full >> u & 1u) vstore<V>(buf + (base + u * kBlock * 16), v[u]);
#pragma unroll
        for (int u = 0; u < kU; ++u)
        {
            const uint32_t p = base + u * kBlock * 16;
            if (p >= end) continue;
            if (!(full >> u & 1u))
            {
                // segment tail: fewer than K rows left, row by row
#pragma unroll
                for (int j = 0; j < K; ++j)
                {
                    if (p + j * L >= end) break;
                    const R x = vload<R>(src + so[u][j]);
                    vstore<R>(buf + (p + j * L), x);
                    vstore<R>(dst + to[u][j], x);
                }
                continue;
            }
            if (drun >> u & 1u)
                vstore<v4_a4>(dst + to[u][0], v4_a4{v[u].x, v[u].y, v[u].z, v[u].w});
            else
            {
                R w[K];
                split<L>(v[u], w);
#pragma unroll
                for (int j = 0; j < K; ++j) vstore<R>(dst + to[u][j], w[j]);
            }
        }
    }
}

// One tile record per workgroup at its block index (grid-stride beyond the grid cap). RUNS: every
// segment of the plan takes the run path (uput_plan::execute_self decides with the launch's
// pointers). Field slot f of either side at field_ptr[f], buffer slot b at buf_ptr[b].
template<bool RUNS>
__global__ __launch_bounds__(kBlock) void k_self_u(kargs a)
{
    const seg_up* __restrict__ recs = static_cast<const seg_up*>(a.tile_recs);
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x)
    {
        const seg_up s = recs[t];
        const uint32_t start = s.first_tile * s.tile_bytes;
        const uint32_t end = min(start + s.tile_bytes, s.bytes);
        const char* src = reinterpret_cast<const char*>(a.field_ptr[s.src_slot]);
        char* dst = reinterpret_cast<char*>(a.field_ptr[s.dst_slot]);
        char* buf = reinterpret_cast<char*>(a.buf_ptr[s.buf_slot] + s.buf_off);
        if constexpr (RUNS)
        {
            if (s.row_bytes == 8) self_runs<8>(s, src, dst, buf, start, end);
            else self_runs<4>(s, src, dst, buf, start, end);
        }
        else
        {
            int w = s.wlog2;
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(src)));
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(dst)));
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(buf)));
            if (s.src_lid64)
            {
                if (s.dst_lid64) self_tile_u_w<true, true>(s, src, dst, buf, start, end, w);
                else self_tile_u_w<true, false>(s, src, dst, buf, start, end, w);
            }
            else if (s.dst_lid64) self_tile_u_w<false, true>(s, src, dst, buf, start, end, w);
            else self_tile_u_w<false, false>(s, src, dst, buf, start, end, w);
        }
    }
}

// Index-list pack that also completes the self messages (the mixed form of an exchange with self
// AND peer list messages): blocks [0, n_self_tiles) take a seg_up record and run k_self_u's tile
// (sending field -> send buffer and receiving field), the next n_peer_tiles a seg_u tile record of
// the peer messages' pack plan and run k_copy<true, seg_u>'s (field -> send buffer). The planner
// (make_umixed) guarantees that no peer tile loads a cell a self tile stores, so the two kinds
// need no order. RUNS: every segment of BOTH parts takes its run path (uput_plan::execute_self
// decides with the launch's pointers). Field slots of both parts at field_ptr, buffer slots at
// buf_ptr.
template<bool RUNS>
__global__ __launch_bounds__(kBlock) void k_pack_self_u(kargs_um a)
{
    const seg_up* __restrict__ self = static_cast<const seg_up*>(a.self_recs);
    const seg_u* __restrict__ peers = static_cast<const seg_u*>(a.peer_recs);
    const uint32_t n_tiles = a.n_self_tiles + a.n_peer_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x)
    {
        if (t < a.n_self_tiles)  // uniform per workgroup
        {
            const seg_up s = self[t];
            const uint32_t start = s.first_tile * s.tile_bytes;
            const uint32_t end = min(start + s.tile_bytes, s.bytes);
            const char* src = reinterpret_cast<const char*>(a.field_ptr[s.src_slot]);
            char* dst = reinterpret_cast<char*>(a.field_ptr[s.dst_slot]);
            char* buf = reinterpret_cast<char*>(a.buf_ptr[s.buf_slot] + s.buf_off);
            if constexpr (RUNS)
            {
                if (s.row_bytes == 8) self_runs<8>(s, src, dst, buf, start, end);
                else self_runs<4>(s, src, dst, buf, start, end);
            }
            else
            {
                int w = s.wlog2;
                w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(src)));
                w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(dst)));
                w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(buf)));
                if (s.src_lid64)
                {
                    if (s.dst_lid64) self_tile_u_w<true, true>(s, src, dst, buf, start, end, w);
                    else self_tile_u_w<true, false>(s, src, dst, buf, start, end, w);
                }
                else if (s.dst_lid64) self_tile_u_w<false, true>(s, src, dst, buf, start, end, w);
                else self_tile_u_w<false, false>(s, src, dst, buf, start, end, w);
            }
            continue;
        }
        const seg_u s = peers[t - a.n_self_tiles];
        const uint32_t start = s.first_tile * s.tile_bytes;
        const uint32_t end = min(start + s.tile_bytes, s.bytes);
        char* field = reinterpret_cast<char*>(a.field_ptr[s.field_slot]);
        char* buf = reinterpret_cast<char*>(a.buf_ptr[s.buf_slot]) + s.buf_off;
        if constexpr (RUNS)
        {
            if (s.row_bytes == 8) copy_runs<true, 8>(s, field, buf, start, end);
            else copy_runs<true, 4>(s, field, buf, start, end);
        }
        else
        {
            int w = s.wlog2;
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(field)));
            w = min(w, ptr_wlog2(reinterpret_cast<uint64_t>(buf)));
            copy_any<true, kU>(s, field, buf, start, end, w);
        }
    }
}

int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        set_error(std::string(what) + " kernel launch failed: " + hipGetErrorString(e));
        return GHX_ERR_HIP;
    }
    return GHX_OK;
}
}  // namespace

void timing_enable(bool on)
{
    if (on && !t_timing) t_timing = new std::vector<std::pair<hipEvent_t, hipEvent_t>>();
    if (!on && t_timing)
    {
        for (auto& e : *t_timing)
        {
            (void)hipEventSynchronize(e.second);
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        delete t_timing;
        t_timing = nullptr;
    }
}

int timing_read(float* ms, int32_t cap, int32_t* n)
{
    int32_t k = 0;
    hipError_t bad = hipSuccess;
    if (t_timing)
    {
        for (auto& e : *t_timing)
        {
            float t = 0.f;
            hipError_t r = hipEventSynchronize(e.second);
            if (r == hipSuccess) r = hipEventElapsedTime(&t, e.first, e.second);
            if (r != hipSuccess && bad == hipSuccess) bad = r;
            if (ms && k < cap) ms[k] = t;
            ++k;
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        t_timing->clear();
    }
    if (n) *n = k;
    if (bad != hipSuccess)
    {
        set_error(std::string("launch timing: ") + hipGetErrorString(bad));
        return GHX_ERR_HIP;
    }
    return GHX_OK;
}

uint32_t grid_for_tiles(uint32_t n_tiles)
{
    uint32_t cap = g_tune.grid_cap > 0 ? uint32_t(g_tune.grid_cap) : (1u << 20);
    return n_tiles < cap ? n_tiles : cap;
}

template<bool REC>
void launch_s(const kargs& a, int direction, hipStream_t s, uint32_t grid)
{
    if (a.parity_word)
    {
        if (direction == 0) launch((k_copy<true, seg_s, false, true, kU, REC>), grid, s, a);
        else launch((k_copy<false, seg_s, false, true, kU, REC>), grid, s, a);
    }
    else if (direction == 0) launch((k_copy<true, seg_s, false, false, kU, REC>), grid, s, a);
    else launch((k_copy<false, seg_s, false, false, kU, REC>), grid, s, a);
}

int launch_structured(const kargs& a, int direction, void* stream, uint32_t grid)
{
    if (a.n_tiles == 0) return GHX_OK;
    grid = min(grid, a.n_tiles);  // k_copy's first tile is unchecked: never more groups than tiles
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.tile_recs) launch_s<true>(a, direction, s, grid);
    else launch_s<false>(a, direction, s, grid);
    return launched("structured");
}

int launch_self(const kargs& a, void* stream, uint32_t grid)
{
    if (a.n_tiles == 0) return GHX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.parity_word)
    {
        if (a.tile_recs) launch((k_self<true, true>), grid, s, a);
        else launch((k_self<true, false>), grid, s, a);
    }
    else if (a.tile_recs) launch((k_self<false, true>), grid, s, a);
    else launch((k_self<false, false>), grid, s, a);
    return launched("self-exchange");
}

int launch_put(const kargs& a, void* stream, uint32_t grid)
{
    if (a.n_tiles == 0) return GHX_OK;
    if (a.tile_recs) launch(k_put<true>, grid, static_cast<hipStream_t>(stream), a);
    else launch(k_put<false>, grid, static_cast<hipStream_t>(stream), a);
    return launched("put");
}

int launch_unpack_x(const kargs& a, void* stream, uint32_t grid)
{
    if (a.n_tiles == 0) return GHX_OK;
    launch(k_unpack_x, min(grid, a.n_tiles), static_cast<hipStream_t>(stream), a);
    return launched("transformed unpack");
}

int launch_pack_x(const kargs& a, void* stream, uint32_t grid)
{
    if (a.n_tiles == 0) return GHX_OK;
    launch(k_pack_x, min(grid, a.n_tiles), static_cast<hipStream_t>(stream), a);
    return launched("transformed reverse pack");
}

int launch_self_cs(const kargs_cs& a, void* stream, uint32_t grid)
{
    const uint32_t n_tiles = a.n_pair_tiles + a.n_x_tiles;
    if (n_tiles == 0) return GHX_OK;
    launch(k_self_cs, min(grid, n_tiles), static_cast<hipStream_t>(stream), a);
    return launched("cubed-sphere self-exchange");
}

int launch_put_cs(const kargs_pcs& a, void* stream, uint32_t grid)
{
    const uint32_t n_tiles = a.n_pair_tiles + a.n_x_tiles;
    if (n_tiles == 0) return GHX_OK;
    launch(k_put_cs, min(grid, n_tiles), static_cast<hipStream_t>(stream), a);
    return launched("cubed-sphere put");
}

int launch_put_u(const kargs& a, void* stream, uint32_t grid, bool runs)
{
    if (a.n_tiles == 0) return GHX_OK;
    grid = min(grid, a.n_tiles);
    if (runs) launch(k_put_u<true>, grid, static_cast<hipStream_t>(stream), a);
    else launch(k_put_u<false>, grid, static_cast<hipStream_t>(stream), a);
    return launched("index-list put");
}

int launch_self_u(const kargs& a, void* stream, uint32_t grid, bool runs)
{
    if (a.n_tiles == 0) return GHX_OK;
    grid = min(grid, a.n_tiles);
    if (runs) launch(k_self_u<true>, grid, static_cast<hipStream_t>(stream), a);
    else launch(k_self_u<false>, grid, static_cast<hipStream_t>(stream), a);
    return launched("index-list self-exchange");
}

int launch_pack_self_u(const kargs_um& a, void* stream, uint32_t grid, bool runs)
{
    const uint32_t n_tiles = a.n_self_tiles + a.n_peer_tiles;
    if (n_tiles == 0) return GHX_OK;
    grid = min(grid, n_tiles);
    if (runs) launch(k_pack_self_u<true>, grid, static_cast<hipStream_t>(stream), a);
    else launch(k_pack_self_u<false>, grid, static_cast<hipStream_t>(stream), a);
    return launched("index-list pack with self messages");
}

template<bool DBL, bool REC>
void launch_u(const kargs& a, int direction, hipStream_t s, uint32_t grid, bool runs)
{
    if (runs && direction == 0) launch((k_copy<true, seg_u, true, DBL, kU, REC>), grid, s, a);
    else if (runs) launch((k_copy<false, seg_u, true, DBL, kU, REC>), grid, s, a);
    else if (direction == 0) launch((k_copy<true, seg_u, false, DBL, kU, REC>), grid, s, a);
    else launch((k_copy<false, seg_u, false, DBL, kU, REC>), grid, s, a);
}

int launch_unstructured(const kargs& a, int direction, void* stream, uint32_t grid, bool runs)
{
    if (a.n_tiles == 0) return GHX_OK;
    grid = min(grid, a.n_tiles);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.parity_word)
    {
        if (a.tile_recs) launch_u<true, true>(a, direction, s, grid, runs);
        else launch_u<true, false>(a, direction, s, grid, runs);
    }
    else if (a.tile_recs) launch_u<false, true>(a, direction, s, grid, runs);
    else launch_u<false, false>(a, direction, s, grid, runs);
    return launched("unstructured");
}

}  // namespace ghx
