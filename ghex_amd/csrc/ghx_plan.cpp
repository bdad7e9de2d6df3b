// ghx_plan.cpp — host-side planner: iteration spaces -> device segment + tile tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "ghx_plan.hpp"

namespace ghx
{
namespace
{
int ctz64(uint64_t v) { return v ? __builtin_ctzll(v) : 64; }

int wlog2_of(uint64_t v)  // log2 of the largest power of two <= 16 dividing v
{
    return std::min(4, ctz64(v));
}

uint32_t tiles_of(uint32_t bytes, uint32_t tb) { return (bytes + tb - 1) / tb; }

// Short-row segments of one field whose rows interleave in memory: row r of `a` and row r-1 of
// `b` share a 128-B line (0 < a.field_off + a.stride[0] - b.field_off < 128, the pieces disjoint).
// For a unit-stride field these are the two x-normal faces (and x-edges) of a halo: the -x piece
// of row y+1 sits right after the +x piece of row y. Returns partner[i] (or -1), symmetric.
std::vector<int32_t> line_partners(const std::vector<seg_s>& segs)
{
    std::vector<int32_t> partner(segs.size(), -1);
    for (size_t i = 0; i < segs.size(); ++i)
    {
        const auto& a = segs[i];
        if (partner[i] >= 0 || a.row_bytes >= g_tune.small_row_bytes ||
            a.n_outer < 1 || a.bytes / a.row_bytes < 2)
            continue;
        for (size_t j = 0; j < segs.size(); ++j)
        {
            if (j == i || partner[j] >= 0) continue;
            const auto& b = segs[j];
            bool same = b.field_slot == a.field_slot && b.row_bytes == a.row_bytes &&
                        b.n_outer == a.n_outer && b.bytes == a.bytes;
            for (int k = 0; same && k < 4; ++k)
                same = b.ext[k] == a.ext[k] && b.stride[k] == a.stride[k];
            if (!same) continue;
            const int64_t d = a.field_off + a.stride[0] - b.field_off;
            if (d <= 0 || d >= 128 || d < int64_t(a.row_bytes)) continue;
            partner[i] = int32_t(j);
            partner[j] = int32_t(i);
            break;
        }
    }
    return partner;
}

std::vector<int32_t> line_partners(const std::vector<seg_u>& segs)
{
    return std::vector<int32_t>(segs.size(), -1);
}

// Rows per tile of a short-row segment. Structured short rows (x-normal faces, edges, corners
// of a unit-stride field) are request-bound: a plan's R short rows are cut so that they make
// about R/128 tiles when each row is one 16-B lane access (16-B rows: H=2 fp64), R/256 otherwise,
// a power of two in [512, 4096] (knob small_tile_rows > 0 overrides). Measured with the
// graph-timed two-launch step over N = 256..640 and H = 1..3 (profiles/r03_tile_rows_sweep.jsonl,
// DESIGN §4): a fixed 4096 rows — the round-1 choice, made at 512^3 H=2 where it still wins — left
// small cubes with a few dozen x-face workgroups (256^3 H=3: 35.4 us vs 14.9 us at 1024 rows) and
// was 15-17 % slower at 512^3 H=1/H=3 than 2048 rows. Index-list gathers are latency-bound
// random accesses and want many workgroups in flight (512 rows), except run-heavy lists on the
// run path, which stream (2048 rows: tools/urun_bench.py, contiguous lids 40 -> 33 us).
// Pack plans whose short rows take several vector accesses each (24-B rows of fp64 at H=3, 12-B
// rows of fp32) cut four times finer (round 6): the pack at 384^3 / 512^3 / 640^3 H=3 takes 12.6 ->
// 11.5 / 19.7 -> 18.5 / 34.3 -> 31.8-33.9 us with 512-row tiles against the old rule's 1024-2048
// rows, 256^3 H=3 equal; single-access rows (H=1, H=2 fp64) keep the old rule, which wins there
// (interleaved A/B, profiles/r06an_pack_tile_rows_ab.jsonl; sweep r06am_pack_tile_rows_sweep.jsonl).
uint32_t short_tile_rows(const seg_s& s, uint64_t short_rows, int dir)
{
    if (dir == 0 && g_tune.pack_tile_rows) return g_tune.pack_tile_rows;
    if (dir == 1 && g_tune.unpack_tile_rows) return g_tune.unpack_tile_rows;
    if (g_tune.small_tile_rows) return g_tune.small_tile_rows;
    // several vector accesses per row (whatever the pointers' alignment allows)
    const bool multi = s.row_bytes > 16 || (s.row_bytes & (s.row_bytes - 1)) != 0;
    const uint64_t want = short_rows / (dir == 0 && multi ? 1024 : s.row_bytes == 16 ? 128 : 256);
    uint32_t r = 512;
    while (r < 4096 && uint64_t(r) * 2 <= want) r *= 2;
    return r;
}
uint32_t short_tile_rows(const seg_u& s, uint64_t, int)
{
    return s.runs == 2 ? g_tune.u_run_tile_rows : g_tune.u_tile_rows;
}
// tile of segments with long rows: structured / unstructured
uint32_t long_tile_bytes(const seg_s&, int dir)
{
    return dir == 1 && g_tune.unpack_tile_bytes ? g_tune.unpack_tile_bytes : g_tune.tile_bytes;
}
uint32_t long_tile_bytes(const seg_u& s, int)
{
    // whole rows per tile (at least one)
    const uint32_t tb = std::max<uint32_t>(g_tune.u_tile_bytes, s.row_bytes);
    return tb - tb % s.row_bytes;
}

// The short form of a segment's field-offset arithmetic (seg_s::amode, field_offset_f in
// ghx_kernels.hip): a row's offset RELATIVE to field_off is computed in 32 bits from full-rate
// 24-bit products (v_mul_u32_u24) with one division per outer dim beyond the last, instead of
// the general form's three divisions and four int64 products (about 16 quarter-rate
// multiplies per vector, the launch's VALU time at small shapes). Exact when every operand of a
// product is below 2^24 and the relative offsets below 2^32: rows, row length, the decoded outer
// extents and the strides (non-negative) of the outer dims in use.
uint8_t short_addressing(const seg_s& s)
{
    if (!g_tune.fast_addr || s.n_outer > 3) return 0;
    constexpr uint64_t k24 = uint64_t(1) << 24;
    const uint64_t rows = s.row_bytes ? s.bytes / s.row_bytes : 0;
    if (rows >= k24 || s.row_bytes >= k24) return 0;
    uint64_t span = s.row_bytes;
    for (int k = 0; k < s.n_outer; ++k)
    {
        if (s.stride[k] < 0 || uint64_t(s.stride[k]) >= k24 || s.ext[k] >= k24) return 0;
        span += uint64_t(s.ext[k] - 1) * uint64_t(s.stride[k]);
    }
    if (span >= (uint64_t(1) << 32)) return 0;
    return s.n_outer == 3 ? 2 : 1;
}

void set_pipe(seg_s& s, bool on) { s.pipe = on ? 1 : 0; }
void set_pipe(seg_u&, bool) {}

// Tile table: per tile {segment, tile index within the segment}. Segments with short rows
// (request-bound: one memory request per row) may use a different tile size from streaming
// segments; the dispatch order of tiles is a tuning knob (hardware dispatches in blockIdx order).
template<typename Seg>
std::vector<uint32_t> build_tiles(std::vector<Seg>& segs, int dir)
{
    std::vector<std::vector<uint32_t>> per(segs.size());
    // each field's short rows (its request-bound work): a field's short-row tiles are sized by
    // its own rows, not the plan's, so a plan of several fields keeps each field's tiling
    // (config 4, five 256^3 fields at H=3: 2048-row tiles by the plan's 686k short rows vs 512
    // by each field's 137k, pack 23.7 -> 21.4 us, profiles/r05_config4_sweep.jsonl)
    std::map<int32_t, uint64_t> short_rows;
    for (const auto& sg : segs)
        if (sg.row_bytes < g_tune.small_row_bytes) short_rows[sg.field_slot] += sg.bytes / sg.row_bytes;
    for (uint32_t i = 0; i < segs.size(); ++i)
    {
        const bool small = segs[i].row_bytes < g_tune.small_row_bytes;
        uint32_t tb = long_tile_bytes(segs[i], dir);
        if (small)
        {
            const uint32_t rows = short_tile_rows(segs[i], short_rows[segs[i].field_slot], dir);
            const uint64_t want = uint64_t(rows) * segs[i].row_bytes;
            tb = uint32_t(std::max<uint64_t>(segs[i].row_bytes, std::min<uint64_t>(want, kMaxTileBytes)));
            tb -= tb % segs[i].row_bytes;  // whole rows per tile
        }
        segs[i].tile_bytes = tb;
        segs[i].fpol = small ? uint8_t(g_tune.short_pol) : uint8_t(0);
        set_pipe(segs[i], !small && dir == 1 && g_tune.unpack_tile_bytes > kTileBytes);
        segs[i].first_tile = 0;
        const uint32_t nt = tiles_of(segs[i].bytes, tb);
        for (uint32_t t = 0; t < nt; ++t) per[i].push_back(t);
    }
    std::vector<uint32_t> out;
    auto emit = [&](uint32_t i, uint32_t t) {
        out.push_back(i);
        out.push_back(t);
    };
    std::vector<uint32_t> idx(segs.size());
    for (uint32_t i = 0; i < segs.size(); ++i) idx[i] = i;
    if (g_tune.order == 1)
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
            return (segs[a].row_bytes < g_tune.small_row_bytes) >
                   (segs[b].row_bytes < g_tune.small_row_bytes);
        });
    std::vector<int32_t> partner(segs.size(), -1);
    if (g_tune.order == 1 && g_tune.xcd_pair) partner = line_partners(segs);
    // Line-sharing pairs first, in lock-step groups of 8 tiles: tile t of one half at block
    // 16k + i, tile t of the other at 16k + 8 + i -> the same XCD (blocks are dealt
    // round-robin over the 8 XCDs) at about the same time, so each shared line is fetched
    // once into that XCD's L2 and both halves' partial writes merge there. A short group is
    // padded with tiles of the other segments so the alignment holds.
    std::vector<std::pair<uint32_t, uint32_t>> rest;
    for (uint32_t i : idx)
        if (partner[i] < 0)
            for (uint32_t t : per[i]) rest.emplace_back(i, t);
    size_t next = 0;
    for (uint32_t i : idx)
    {
        const int32_t j = partner[i];
        if (j < 0 || uint32_t(j) < i) continue;
        const size_t n = per[i].size();  // == per[j].size(): partners have equal bytes
        for (size_t k = 0; k < n; k += 8)
        {
            const size_t m = std::min<size_t>(8, n - k);
            for (size_t u = 0; u < m; ++u) emit(uint32_t(j), per[size_t(j)][k + u]);
            for (size_t u = m; u < 8 && next < rest.size(); ++u, ++next)
                emit(rest[next].first, rest[next].second);
            for (size_t u = 0; u < m; ++u) emit(i, per[i][k + u]);
        }
    }
    for (; next < rest.size(); ++next) emit(rest[next].first, rest[next].second);
    return out;
}

bool have_device()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// Upload a plan's host tables to device memory (synchronous: plan creation is setup time).
// Without a HIP device (the CPU build container) the plan stays host-only: its metadata can be
// inspected, executing it reports GHX_ERR_HIP.
template<typename Seg>
void upload(device_tables& dt, const std::vector<Seg>& segs, const std::vector<uint32_t>& tiles)
{
    dt.release();
    if (segs.empty() || !have_device()) return;
    const size_t sb = segs.size() * sizeof(Seg), tb = tiles.size() * sizeof(uint32_t);
    if (hipMalloc(&dt.segs, sb) != hipSuccess) throw hip_error("hipMalloc(segments)");
    if (hipMalloc(reinterpret_cast<void**>(&dt.tiles), tb) != hipSuccess)
        throw hip_error("hipMalloc(tiles)");
    if (hipMemcpy(dt.segs, segs.data(), sb, hipMemcpyHostToDevice) != hipSuccess)
        throw hip_error("hipMemcpy(segments)");
    if (hipMemcpy(dt.tiles, tiles.data(), tb, hipMemcpyHostToDevice) != hipSuccess)
        throw hip_error("hipMemcpy(tiles)");
    if (g_tune.tile_records && !tiles.empty())
    {
        // one record per tile, in dispatch order: the tile's segment with first_tile = the
        // tile's index in it (a workgroup loads its record from blockIdx alone)
        std::vector<Seg> rec(tiles.size() / 2);
        for (size_t t = 0; t < rec.size(); ++t)
        {
            rec[t] = segs[tiles[2 * t]];
            rec[t].first_tile = tiles[2 * t + 1];
        }
        const size_t rb = rec.size() * sizeof(Seg);
        if (hipMalloc(&dt.recs, rb) != hipSuccess) throw hip_error("hipMalloc(tile records)");
        if (hipMemcpy(dt.recs, rec.data(), rb, hipMemcpyHostToDevice) != hipSuccess)
            throw hip_error("hipMemcpy(tile records)");
    }
}
// Cut segments (in order) into launch groups of at most GHX_MAX_SLOTS distinct field and buffer
// slots each; local[k] = segment k's slots inside its group. One group with identity maps
// (empty) when every caller slot is already below GHX_MAX_SLOTS.
struct slot_partition
{
    std::vector<std::vector<uint32_t>> segs;
    std::vector<std::vector<int32_t>> fmap, bmap;
    std::vector<int32_t> lf, lb;
};

slot_partition partition_slots(const std::vector<int32_t>& gf, const std::vector<int32_t>& gb)
{
    slot_partition p;
    const size_t n = gf.size();
    p.lf = gf;
    p.lb = gb;
    int32_t mf = -1, mb = -1;
    for (size_t k = 0; k < n; ++k)
    {
        mf = std::max(mf, gf[k]);
        mb = std::max(mb, gb[k]);
    }
    if (mf < GHX_MAX_SLOTS && mb < GHX_MAX_SLOTS)
    {
        p.segs.emplace_back();
        for (size_t k = 0; k < n; ++k) p.segs[0].push_back(uint32_t(k));
        p.fmap.emplace_back();
        p.bmap.emplace_back();
        return p;
    }
    std::map<int32_t, int32_t> cf, cb;  // current group: caller slot -> local slot
    for (size_t k = 0; k < n; ++k)
    {
        const bool nf = !cf.count(gf[k]), nb = !cb.count(gb[k]);
        if (p.segs.empty() || cf.size() + nf > size_t(GHX_MAX_SLOTS) ||
            cb.size() + nb > size_t(GHX_MAX_SLOTS))
        {
            p.segs.emplace_back();
            p.fmap.emplace_back();
            p.bmap.emplace_back();
            cf.clear();
            cb.clear();
        }
        auto slot = [](std::map<int32_t, int32_t>& m, std::vector<int32_t>& map, int32_t g) {
            auto it = m.find(g);
            if (it != m.end()) return it->second;
            const int32_t l = int32_t(map.size());
            m.emplace(g, l);
            map.push_back(g);
            return l;
        };
        p.lf[k] = slot(cf, p.fmap.back(), gf[k]);
        p.lb[k] = slot(cb, p.bmap.back(), gb[k]);
        p.segs.back().push_back(uint32_t(k));
    }
    return p;
}

// The launch groups of a plan's segments (gf / gb: the caller's slots of each): the partition,
// each group's segments with their local slots, its tile table and its device tables.
template<typename Seg>
std::vector<launch_group<Seg>> build_groups(const std::vector<Seg>& segs, const std::vector<int32_t>& gf,
                                            const std::vector<int32_t>& gb, int direction)
{
    slot_partition part = partition_slots(gf, gb);
    std::vector<launch_group<Seg>> groups(part.segs.size());
    for (size_t g = 0; g < groups.size(); ++g)
    {
        launch_group<Seg>& grp = groups[g];
        grp.fmap = std::move(part.fmap[g]);
        grp.bmap = std::move(part.bmap[g]);
        for (uint32_t k : part.segs[g])
        {
            Seg x = segs[k];
            x.field_slot = uint16_t(part.lf[k]);
            x.buf_slot = uint16_t(part.lb[k]);
            grp.host_segs.push_back(x);
        }
        grp.host_tiles = build_tiles(grp.host_segs, direction);
        grp.n_tiles = uint32_t(grp.host_tiles.size() / 2);
        upload(grp.dev, grp.host_segs, grp.host_tiles);
    }
    return groups;
}

// A plan's execution: one launch per group that has tiles, in order on one stream. Per group the
// kargs hold its device tables, the caller's pointers through its slot maps and, where the plan
// has double-buffered buffers, their parity; `launch(kargs, group)` is the plan's kernel launch.
template<typename Plan, typename Launch>
int execute_groups(const Plan& p, const parity_cfg* parity, void* const* fptr, int nf,
                   void* const* bptr, int nb, Launch&& launch)
{
    if (total_tiles(p.groups) == 0) return GHX_OK;
    if (nf <= p.max_field_slot || nb <= p.max_buf_slot)
        throw invalid("pointer arrays do not cover the plan's slots");
    int rc = GHX_OK;
    for (size_t g = 0; rc == GHX_OK && g < p.groups.size(); ++g)
    {
        const auto& grp = p.groups[g];
        if (grp.n_tiles == 0) continue;
        if (!grp.dev.segs && !grp.dev.recs)
            throw hip_error("plan has no device tables (no HIP device at creation)");
        kargs a{};
        a.segs = grp.dev.segs;
        a.tile_seg = grp.dev.tiles;
        a.tile_recs = grp.dev.recs;
        a.n_tiles = grp.n_tiles;
        fill_slots(a.field_ptr, fptr, grp.fmap, p.max_field_slot + 1, "field");
        fill_slots(a.buf_ptr, bptr, grp.bmap, p.max_buf_slot + 1, "buffer");
        if (parity) parity->apply(a, grp.bmap, p.max_buf_slot + 1);
        rc = launch(a, grp);
    }
    return rc;
}
}  // namespace

void fill_slots(uint64_t* dst, void* const* src, const std::vector<int32_t>& map, int n_identity,
                const char* what)
{
    const int n = map.empty() ? n_identity : int(map.size());
    for (int i = 0; i < n; ++i)
    {
        void* p = src[map.empty() ? i : map[size_t(i)]];
        if (!p) throw invalid(std::string("null ") + what + " pointer");
        dst[i] = reinterpret_cast<uint64_t>(p);
    }
}

void device_tables::release()
{
    if (segs) (void)hipFree(segs);
    if (tiles) (void)hipFree(tiles);
    if (recs) (void)hipFree(recs);
    if (lids) (void)hipFree(lids);
    segs = nullptr;
    tiles = nullptr;
    recs = nullptr;
    lids = nullptr;
}

void upload_segments(device_tables& dt, const std::vector<seg_s>& segs)
{
    dt.release();
    if (segs.empty() || !have_device()) return;
    const size_t sb = segs.size() * sizeof(seg_s);
    if (hipMalloc(&dt.segs, sb) != hipSuccess) throw hip_error("hipMalloc(segments)");
    if (hipMemcpy(dt.segs, segs.data(), sb, hipMemcpyHostToDevice) != hipSuccess)
        throw hip_error("hipMemcpy(segments)");
}

std::vector<seg_s> pair_records(const std::vector<seg_s>& primary, const std::vector<seg_s>& companion,
                                const std::vector<uint32_t>& tiles)
{
    std::vector<seg_s> rec(tiles.size());  // 2 per tile
    for (size_t t = 0; t < tiles.size() / 2; ++t)
    {
        const uint32_t si = tiles[2 * t];
        rec[2 * t] = primary[si];
        rec[2 * t].first_tile = tiles[2 * t + 1];
        rec[2 * t + 1] = companion[si];
    }
    return rec;
}

void upload_pair_records(device_tables& dt, const std::vector<seg_s>& primary,
                         const std::vector<seg_s>& companion, const std::vector<uint32_t>& tiles)
{
    dt.release();
    if (!g_tune.tile_records || tiles.empty() || !have_device()) return;
    if (primary.size() != companion.size()) throw invalid("pair records: segment counts differ");
    const std::vector<seg_s> rec = pair_records(primary, companion, tiles);
    const size_t rb = rec.size() * sizeof(seg_s);
    if (hipMalloc(&dt.recs, rb) != hipSuccess) throw hip_error("hipMalloc(pair records)");
    if (hipMemcpy(dt.recs, rec.data(), rb, hipMemcpyHostToDevice) != hipSuccess)
        throw hip_error("hipMemcpy(pair records)");
}

// ---------------------------------------------------------------------------------------------
// structured
// ---------------------------------------------------------------------------------------------
void validate_field(const ghx_field_desc& f)
{
    if (f.dim < 1 || f.dim > GHX_MAX_DIM) throw invalid("field dim must be in [1, 4]");
    if (f.elem_size < 1) throw invalid("elem_size must be >= 1");
    if (f.num_components < 1) throw invalid("number of components must be greater than 0");
    if (!f.has_components && f.num_components > 1)
        throw invalid("this field cannot have more than 1 components");
    if (f.has_components && f.dim < 2) throw invalid("component axis needs dim >= 2");
    bool seen[GHX_MAX_DIM] = {false, false, false, false};
    for (int d = 0; d < f.dim; ++d)
    {
        if (f.layout[d] < 0 || f.layout[d] >= f.dim || seen[f.layout[d]])
            throw invalid("layout must be a permutation of 0..dim-1");
        seen[f.layout[d]] = true;
    }
}

// Append the segments of one iteration space (`box`, spatial dims only).
// Mirrors make_pack_is / make_buffer_desc / make_is (regular/field_descriptor.hpp:114-150):
// the buffer box is dense in the field's layout order; row = run along the layout's stride-1
// dim. Returns the buffer bytes of the space (is.size() * num_components * sizeof(T)).
uint64_t add_box_segments(std::vector<seg_s>& out, const ghx_field_desc& f, const ghx_box& box,
                          uint16_t field_slot, uint16_t buf_slot, uint64_t buf_off)
{
    const int D = f.dim;
    const int spatial = D - (f.has_components ? 1 : 0);
    int64_t first[GHX_MAX_DIM], ext[GHX_MAX_DIM];
    for (int d = 0; d < D; ++d)
    {
        if (d < spatial)
        {
            first[d] = box.first[d];
            ext[d] = int64_t(box.last[d]) - box.first[d] + 1;
        }
        else
        {
            first[d] = 0;
            ext[d] = f.num_components;
        }
        if (ext[d] <= 0) throw invalid("iteration space: first must be <= last");
        // bounds against the declared extents (the reference does not check; a GPU fault here
        // would take the whole node down, so the planner refuses instead)
        const int64_t off = d < spatial ? f.offsets[d] : 0;
        if (f.extents[d] > 0 && (first[d] + off < 0 || first[d] + ext[d] - 1 + off >= f.extents[d]))
            throw invalid("iteration space outside the field extents");
    }
    int64_t n = 1;
    for (int d = 0; d < D; ++d) n *= ext[d];
    const int64_t elem = f.elem_size;
    // dims sorted by layout value, fastest (value D-1) first
    int by_speed[GHX_MAX_DIM];
    for (int d = 0; d < D; ++d) by_speed[D - 1 - f.layout[d]] = d;
    const int cont = by_speed[0];
    int64_t L;
    int outer[GHX_MAX_DIM + 1];
    int n_outer = 0;
    if (f.byte_strides[cont] == elem)
    {
        L = ext[cont] * elem;
        for (int k = 1; k < D; ++k) outer[n_outer++] = by_speed[k];
    }
    else
    {
        // strided fastest dim: every element is its own row (element-wise semantics of the GPU
        // reference, pack_kernels.hpp:161-183)
        L = elem;
        for (int k = 0; k < D; ++k) outer[n_outer++] = by_speed[k];
    }
    int64_t ostride[GHX_MAX_DIM], oext[GHX_MAX_DIM];
    for (int k = 0; k < n_outer; ++k)
    {
        ostride[k] = f.byte_strides[outer[k]];
        oext[k] = ext[outer[k]];
    }
    // merge rows that are contiguous in the field too (box spans the full padded run)
    while (n_outer > 0 && ostride[0] == L && oext[0] * L < (int64_t(1) << 30))
    {
        L *= oext[0];
        for (int k = 1; k < n_outer; ++k)
        {
            ostride[k - 1] = ostride[k];
            oext[k - 1] = oext[k];
        }
        --n_outer;
    }
    if (n_outer > 4) throw invalid("too many outer dims");
    if (L >= (int64_t(1) << 31)) throw invalid("row too long");
    int64_t field_off = 0;
    for (int d = 0; d < D; ++d)
    {
        const int64_t off = d < spatial ? f.offsets[d] : 0;
        field_off += (first[d] + off) * f.byte_strides[d];
    }
    // split along the slowest outer dim so that one segment stays below 2^31 bytes
    int64_t rows_per_slowest = 1;
    for (int k = 0; k + 1 < n_outer; ++k) rows_per_slowest *= oext[k];
    const int64_t slab = rows_per_slowest * L;  // bytes per unit of the slowest outer dim
    const int64_t nslow = n_outer > 0 ? oext[n_outer - 1] : 1;
    const int64_t max_bytes = (int64_t(1) << 31) - kMaxTileBytes;
    int64_t chunk = n_outer > 0 ? std::max<int64_t>(1, max_bytes / slab) : 1;
    if (n_outer == 0 && L > max_bytes) throw invalid("segment too large");
    if (n_outer > 0 && slab > max_bytes) throw invalid("segment row block too large");
    for (int64_t s0 = 0; s0 < nslow; s0 += chunk)
    {
        const int64_t cnt = std::min(chunk, nslow - s0);
        seg_s s{};
        s.field_slot = field_slot;
        s.buf_slot = buf_slot;
        s.row_bytes = uint32_t(L);
        s.n_outer = uint8_t(n_outer);
        int64_t rows = 1;
        for (int k = 0; k < 4; ++k)
        {
            if (k < n_outer)
            {
                s.stride[k] = ostride[k];
                s.ext[k] = uint32_t(k == n_outer - 1 ? cnt : oext[k]);
            }
            else
            {
                s.stride[k] = 0;
                s.ext[k] = 1;
            }
            rows *= s.ext[k];
        }
        s.field_off = field_off + (n_outer > 0 ? s0 * ostride[n_outer - 1] : 0);
        s.buf_off = buf_off + uint64_t(s0 * slab);
        s.bytes = uint32_t(rows * L);
        s.mag_row = make_magic(uint32_t(L));
        for (int k = 0; k < 3; ++k) s.mag_ext[k] = make_magic(s.ext[k]);
        const int wb = std::min(wlog2_of(uint64_t(L)), wlog2_of(s.buf_off));  // buffer side
        int wf = wlog2_of(uint64_t(s.field_off));                             // field side
        for (int k = 0; k < n_outer; ++k)
            if (s.ext[k] > 1) wf = std::min(wf, wlog2_of(uint64_t(s.stride[k] < 0 ? -s.stride[k] : s.stride[k])));
        s.wlog2 = uint8_t(std::min(wb, wf));
        s.amode = short_addressing(s);
        out.push_back(s);
    }
    return uint64_t(n * elem);
}

splan::splan(const ghx_pack_entry* entries, int n_entries, int dir) : direction(dir)
{
    tile_bytes = g_tune.tile_bytes;
    if (dir != 0 && dir != 1) throw invalid("direction must be 0 (pack) or 1 (unpack)");
    std::vector<seg_s> segs;
    std::vector<int32_t> gf, gb;  // caller slots per segment
    for (int e = 0; e < n_entries; ++e)
    {
        const auto& en = entries[e];
        validate_field(en.field);
        if (en.field_slot < 0 || en.buffer_slot < 0) throw invalid("negative slot");
        if (en.n_boxes < 0 || (en.n_boxes > 0 && !en.boxes)) throw invalid("bad boxes");
        max_field_slot = std::max(max_field_slot, en.field_slot);
        max_buf_slot = std::max(max_buf_slot, en.buffer_slot);
        uint64_t off = en.buffer_offset;
        for (int b = 0; b < en.n_boxes; ++b)
            off += add_box_segments(segs, en.field, en.boxes[b], 0, 0, off);
        gf.resize(segs.size(), en.field_slot);
        gb.resize(segs.size(), en.buffer_slot);
        bytes += off - en.buffer_offset;
    }
    n_segments = int32_t(segs.size());
    groups = build_groups(segs, gf, gb, direction);
}

splan::splan(std::vector<seg_s> segs, const std::vector<int32_t>& gf, const std::vector<int32_t>& gb,
             uint64_t nbytes, int dir)
: direction(dir)
{
    tile_bytes = g_tune.tile_bytes;
    if (dir != 0 && dir != 1) throw invalid("direction must be 0 (pack) or 1 (unpack)");
    if (gf.size() != segs.size() || gb.size() != segs.size()) throw invalid("one slot pair per segment");
    for (size_t k = 0; k < segs.size(); ++k)
    {
        if (gf[k] < 0 || gb[k] < 0) throw invalid("negative slot");
        max_field_slot = std::max(max_field_slot, gf[k]);
        max_buf_slot = std::max(max_buf_slot, gb[k]);
    }
    bytes = nbytes;
    n_segments = int32_t(segs.size());
    groups = build_groups(segs, gf, gb, direction);
}

int splan::execute(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const
{
    return execute_groups(*this, &parity, fptr, nf, bptr, nb,
                          [&](const kargs& a, const launch_group<seg_s>&) {
                              return launch_structured(a, direction, stream, grid_for_tiles(a.n_tiles));
                          });
}

void finish_segment(seg_s& s)
{
    s.mag_row = make_magic(s.row_bytes);
    for (int k = 0; k < 3; ++k) s.mag_ext[k] = make_magic(s.ext[k]);
    const int wb = std::min(wlog2_of(uint64_t(s.row_bytes)), wlog2_of(s.buf_off));
    int wf = wlog2_of(uint64_t(s.field_off));
    for (int k = 0; k < s.n_outer; ++k)
        if (s.ext[k] > 1) wf = std::min(wf, wlog2_of(uint64_t(s.stride[k] < 0 ? -s.stride[k] : s.stride[k])));
    s.wlog2 = uint8_t(std::min(wb, wf));
    s.amode = short_addressing(s);
}

// ---------------------------------------------------------------------------------------------
// transformed unpack (cubed sphere)
// ---------------------------------------------------------------------------------------------
// Tile shape: about tile_elems elements (one per lane) as a sub-box that is wide along both
// the buffer's fastest axis (coalesced reads) and the field's fastest axis (whole field runs per
// wave store): up to 16 elements of the field's axis first, the rest of the budget along the
// buffer's, what is left back to the field's and then to the other axes in buffer order; the
// chunks of an axis are evened out. When the two axes coincide (only a component is negated)
// the axes are filled in buffer order. The store side walks the tile with its axes sorted by
// ascending |field stride| (axes of extent 1 last).
void make_tile_records(std::vector<seg_x>& out, const xseg& b, uint16_t field_slot,
                       uint16_t buf_slot, std::vector<xtile_pos>* where)
{
    if (b.elem < 1 || b.elem > 16 || (b.elem & (b.elem - 1))) throw invalid("transformed segment: element size");
    if (b.bytes() == 0 || b.bytes() >= (uint64_t(1) << 31)) throw invalid("transformed segment: box size");
    auto mag = [&](int k) { return uint64_t(b.stride[k] < 0 ? -b.stride[k] : b.stride[k]); };
    const uint64_t budget = std::max<uint32_t>(1, b.tile_elems);
    uint32_t t[4] = {1, 1, 1, 1};
    int ba = -1, fa = -1;
    for (int k = 0; k < 4; ++k)
    {
        if (b.ext[k] <= 1) continue;
        if (ba < 0) ba = k;
        if (fa < 0 || mag(k) < mag(fa)) fa = k;
    }
    uint64_t room = budget;
    if (ba >= 0 && fa != ba)
    {
        t[fa] = uint32_t(std::min<uint64_t>(b.ext[fa], 16));
        t[ba] = uint32_t(std::min<uint64_t>(b.ext[ba], std::max<uint64_t>(1, budget / t[fa])));
        t[fa] = uint32_t(std::min<uint64_t>(b.ext[fa], std::max<uint64_t>(1, budget / t[ba])));
        room = std::max<uint64_t>(1, budget / (uint64_t(t[fa]) * t[ba]));
    }
    for (int k = 0; k < 4; ++k)
    {
        if (ba >= 0 && fa != ba && (k == fa || k == ba)) continue;
        t[k] = uint32_t(std::min<uint64_t>(b.ext[k], std::max<uint64_t>(1, room)));
        room = std::max<uint64_t>(1, room / t[k]);
    }
    for (int k = 0; k < 4; ++k)
    {
        const uint32_t chunks = (b.ext[k] + t[k] - 1) / t[k];
        t[k] = (b.ext[k] + chunks - 1) / chunks;
    }
    int perm[4] = {0, 1, 2, 3};
    std::stable_sort(perm, perm + 4, [&](int x, int y) {
        if ((t[x] == 1) != (t[y] == 1)) return t[y] == 1;
        return mag(x) < mag(y);
    });
    const uint32_t bs[4] = {1, b.ext[0], b.ext[0] * b.ext[1], b.ext[0] * b.ext[1] * b.ext[2]};
    int elog2 = 0;
    while ((1u << elog2) < b.elem) ++elog2;
    uint32_t o[4];
    for (o[3] = 0; o[3] < b.ext[3]; o[3] += t[3])
        for (o[2] = 0; o[2] < b.ext[2]; o[2] += t[2])
            for (o[1] = 0; o[1] < b.ext[1]; o[1] += t[1])
                for (o[0] = 0; o[0] < b.ext[0]; o[0] += t[0])
                {
                    seg_x r{};
                    r.field_off = b.field_off;
                    uint64_t lin = 0, n = 1;
                    for (int k = 3; k >= 0; --k) lin = lin * b.ext[k] + o[k];
                    for (int k = 0; k < 4; ++k) r.field_off += int64_t(o[k]) * b.stride[k];
                    r.buf_off = b.buf_off + lin * b.elem;
                    r.comp_pos = 4;
                    for (int j = 0; j < 4; ++j)
                    {
                        const int k = perm[j];
                        r.stride[j] = b.stride[k];
                        r.tdim[j] = t[k];
                        r.act[j] = std::min(t[k], b.ext[k] - o[k]);
                        r.bstride[j] = bs[k];
                        r.mag[j] = make_magic(t[k]);
                        n *= r.act[j];
                        if (k == b.comp_axis) r.comp_pos = uint8_t(j);
                    }
                    r.bytes = uint32_t(n * b.elem);
                    r.comp0 = b.comp_axis >= 0 ? o[b.comp_axis] : 0;
                    r.field_slot = field_slot;
                    r.buf_slot = buf_slot;
                    r.elog2 = uint8_t(elog2);
                    r.neg_mask = b.neg_mask;
                    r.neg_kind = b.neg_kind;
                    out.push_back(r);
                    if (where)
                    {
                        xtile_pos w{};
                        for (int k = 0; k < 4; ++k)
                        {
                            w.origin[k] = o[k];
                            w.axis[k] = perm[k];
                        }
                        where->push_back(w);
                    }
                }
}

xplan::xplan(std::vector<xseg> bx) : boxes(std::move(bx))
{
    std::vector<int32_t> gf, gb;
    for (const xseg& b : boxes)
    {
        if (b.field_slot < 0 || b.buf_slot < 0) throw invalid("negative slot");
        max_field_slot = std::max(max_field_slot, b.field_slot);
        max_buf_slot = std::max(max_buf_slot, b.buf_slot);
        gf.push_back(b.field_slot);
        gb.push_back(b.buf_slot);
        bytes += b.bytes();
    }
    n_records = int32_t(boxes.size());
    slot_partition part = partition_slots(gf, gb);
    groups = std::vector<launch_group<seg_x>>(part.segs.size());
    for (size_t g = 0; g < groups.size(); ++g)
    {
        launch_group<seg_x>& grp = groups[g];
        grp.fmap = std::move(part.fmap[g]);
        grp.bmap = std::move(part.bmap[g]);
        for (uint32_t k : part.segs[g])
            make_tile_records(grp.host_segs, boxes[k], uint16_t(part.lf[k]), uint16_t(part.lb[k]));
        grp.n_tiles = uint32_t(grp.host_segs.size());
        n_tiles += grp.n_tiles;
        if (grp.n_tiles && have_device())
        {
            const size_t rb = grp.host_segs.size() * sizeof(seg_x);
            if (hipMalloc(&grp.dev.recs, rb) != hipSuccess) throw hip_error("hipMalloc(transformed records)");
            if (hipMemcpy(grp.dev.recs, grp.host_segs.data(), rb, hipMemcpyHostToDevice) != hipSuccess)
                throw hip_error("hipMemcpy(transformed records)");
        }
    }
}

int xplan::execute(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const
{
    return execute_groups(*this, nullptr, fptr, nf, bptr, nb,
                          [&](const kargs& a, const launch_group<seg_x>&) {
                              return launch_unpack_x(a, stream, grid_for_tiles(a.n_tiles));
                          });
}

int xplan::execute_pack(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const
{
    return execute_groups(*this, nullptr, fptr, nf, bptr, nb,
                          [&](const kargs& a, const launch_group<seg_x>&) {
                              return launch_pack_x(a, stream, grid_for_tiles(a.n_tiles));
                          });
}

// ---------------------------------------------------------------------------------------------
// fused cubed-sphere self exchange and cubed-sphere put
// ---------------------------------------------------------------------------------------------
// Pair records of segments that already carry their slots: tile sizes, cache policies and the
// dispatch order are the ordinary plans' (build_tiles, under the caller's g_tune.tile_bytes); the
// launch is tiled by the primary side's table alone, as k_self and k_put are.
void cs_records::build_pairs(std::vector<seg_s> p, std::vector<seg_s> q)
{
    if (p.empty()) return;
    const std::vector<uint32_t> tiles = build_tiles(p, 0);
    (void)build_tiles(q, 1);
    pair_recs = pair_records(p, q, tiles);
}

// The tile records of the spaces that do not pair: make_tile_records of the receiving side, each
// with the sending side of the same cells. `buffered`: the records keep the box's buffer slot
// (a put has no buffer: slot 0).
void cs_records::build_tiles_x(const std::vector<xsbox>& boxes, bool buffered)
{
    for (const xsbox& b : boxes)
    {
        std::vector<seg_x> recs;
        std::vector<xtile_pos> where;
        make_tile_records(recs, b.dst, uint16_t(b.dst.field_slot),
                          uint16_t(buffered ? b.dst.buf_slot : 0), &where);
        for (size_t t = 0; t < recs.size(); ++t)
        {
            seg_xs r{};
            r.x = recs[t];
            r.src_off = b.src_off;
            for (int k = 0; k < 4; ++k) r.src_off += int64_t(where[t].origin[k]) * b.src_stride[k];
            for (int j = 0; j < 4; ++j) r.src_stride[j] = b.src_stride[where[t].axis[j]];
            r.src_slot = uint16_t(b.src_slot);
            x_recs.push_back(r);
        }
        ++n_x_records;
    }
}

// both tables to device memory (dev.segs: pair_recs, dev.recs: x_recs; a no-op without a device)
void cs_records::upload(const char* what)
{
    if (!have_device()) return;
    auto up = [&](void*& to, const void* from, size_t nb, const char* table) {
        if (nb == 0) return;
        const std::string name = std::string("(") + what + " " + table + " records)";
        if (hipMalloc(&to, nb) != hipSuccess) throw hip_error("hipMalloc" + name);
        if (hipMemcpy(to, from, nb, hipMemcpyHostToDevice) != hipSuccess) throw hip_error("hipMemcpy" + name);
    };
    up(dev.segs, pair_recs.data(), pair_recs.size() * sizeof(seg_s), "pair");
    up(dev.recs, x_recs.data(), x_recs.size() * sizeof(seg_xs), "tile");
}

void cs_records::check_tables() const
{
    if ((!pair_recs.empty() && !dev.segs) || (!x_recs.empty() && !dev.recs))
        throw hip_error("plan has no device tables (no HIP device at creation)");
}

cs_self_plan::cs_self_plan(const std::vector<seg_s>& pack, const std::vector<seg_s>& unpack,
                           const std::vector<int32_t>& gf_p, const std::vector<int32_t>& gf_u,
                           const std::vector<int32_t>& gb, const std::vector<xsbox>& boxes)
{
    if (pack.size() != unpack.size() || gf_p.size() != pack.size() || gf_u.size() != pack.size() ||
        gb.size() != pack.size())
        throw invalid("self plan: one unpack segment and one slot triple per pack segment");
    auto slot = [&](int32_t f, int32_t b) {
        if (f < 0 || b < 0) throw invalid("negative slot");
        max_field_slot = std::max(max_field_slot, f);
        max_buf_slot = std::max(max_buf_slot, b);
        if (max_field_slot + 1 + max_buf_slot + 1 > kCsSelfPtrs)
            throw invalid("more field and buffer slots than the fused launch's arguments hold");
    };
    std::vector<seg_s> p = pack, q = unpack;
    for (size_t k = 0; k < pack.size(); ++k)
    {
        slot(gf_p[k], gb[k]);
        slot(gf_u[k], gb[k]);
        p[k].field_slot = uint16_t(gf_p[k]);
        q[k].field_slot = uint16_t(gf_u[k]);
        p[k].buf_slot = q[k].buf_slot = uint16_t(gb[k]);
    }
    for (const xsbox& b : boxes)
    {
        slot(b.dst.field_slot, b.dst.buf_slot);
        slot(b.src_slot, b.dst.buf_slot);
    }
    // the fused self exchange's tile size, as ghx_exchange_self uses it
    {
        const tile_bytes_scope tile(g_tune.self_tile_bytes);
        build_pairs(std::move(p), std::move(q));
    }
    build_tiles_x(boxes, true);
    upload("self");
}

int cs_self_plan::execute(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const
{
    const uint32_t nt = n_pair_tiles() + n_x_tiles();
    if (nt == 0) return GHX_OK;
    if (nf <= max_field_slot || nb <= max_buf_slot) throw invalid("pointer arrays do not cover the plan's slots");
    check_tables();
    kargs_cs a{};
    a.pair_recs = dev.segs;
    a.x_recs = dev.recs;
    a.n_pair_tiles = n_pair_tiles();
    a.n_x_tiles = n_x_tiles();
    a.buf_base = uint32_t(max_field_slot + 1);
    fill_slots(a.ptr, fptr, {}, max_field_slot + 1, "field");
    fill_slots(a.ptr + a.buf_base, bptr, {}, max_buf_slot + 1, "buffer");
    return launch_self_cs(a, stream, grid_for_tiles(nt));
}

cs_put_plan::cs_put_plan(const std::vector<seg_s>& from, const std::vector<seg_s>& to,
                         const std::vector<int32_t>& gs, const std::vector<int32_t>& gd,
                         const std::vector<xsbox>& boxes, uint64_t nbytes)
: bytes(nbytes)
{
    if (from.size() != to.size() || gs.size() != from.size() || gd.size() != from.size())
        throw invalid("put plan: one target segment and one slot pair per source segment");
    auto slot = [&](int32_t s, int32_t d) {
        if (s < 0 || d < 0) throw invalid("negative slot");
        if (s >= GHX_MAX_SLOTS || d >= GHX_MAX_SLOTS)
            throw invalid("a put plan takes at most 64 source and 64 target fields (one launch)");
        max_src_slot = std::max(max_src_slot, s);
        max_dst_slot = std::max(max_dst_slot, d);
    };
    std::vector<seg_s> p = from, q = to;
    for (size_t k = 0; k < from.size(); ++k)
    {
        slot(gs[k], gd[k]);
        p[k].field_slot = uint16_t(gs[k]);
        q[k].field_slot = uint16_t(gd[k]);
    }
    for (const xsbox& b : boxes) slot(b.src_slot, b.dst.field_slot);
    // the pack plans' tile sizes, as ghx_put_create's plans have
    build_pairs(std::move(p), std::move(q));
    build_tiles_x(boxes, false);
    upload("put");
}

int cs_put_plan::execute(void* const* src, int ns, void* const* dst, int nd, void* stream) const
{
    const uint32_t nt = n_pair_tiles() + n_x_tiles();
    if (nt == 0) return GHX_OK;
    if (ns <= max_src_slot || nd <= max_dst_slot) throw invalid("pointer arrays do not cover the plan's slots");
    check_tables();
    if (x_recs.empty())
    {
        // nothing to transform: k_put's record form over the pair records
        kargs k{};
        k.tile_recs = dev.segs;
        k.n_tiles = n_pair_tiles();
        fill_slots(k.field_ptr, src, {}, max_src_slot + 1, "source field");
        fill_slots(k.buf_ptr, dst, {}, max_dst_slot + 1, "target field");
        return launch_put(k, stream, grid_for_tiles(k.n_tiles));
    }
    kargs_pcs a{};
    a.pair_recs = dev.segs;
    a.x_recs = dev.recs;
    a.n_pair_tiles = n_pair_tiles();
    a.n_x_tiles = n_x_tiles();
    fill_slots(a.src_ptr, src, {}, max_src_slot + 1, "source field");
    fill_slots(a.dst_ptr, dst, {}, max_dst_slot + 1, "target field");
    return launch_put_cs(a, stream, grid_for_tiles(nt));
}

// ---------------------------------------------------------------------------------------------
// unstructured
// ---------------------------------------------------------------------------------------------
uplan::uplan(const ghx_upack_entry* entries, int n_entries, int dir) : direction(dir)
{
    tile_bytes = g_tune.tile_bytes;
    if (dir != 0 && dir != 1) throw invalid("direction must be 0 (pack) or 1 (unpack)");
    std::vector<seg_u> segs;
    // all index lists in one device allocation: int32 where they fit
    struct pending
    {
        size_t seg;
        size_t off;  // the segment's list in the device allocation
    };
    struct lid_upload
    {
        const int64_t* lids;
        int64_t n;
        bool wide;
        size_t off;
    };
    std::vector<pending> pend;
    std::vector<lid_upload> uploads;
    std::map<std::pair<const int64_t*, int64_t>, size_t> lid_off;
    std::vector<int32_t> gf, gb;  // caller slots per segment
    size_t lid_bytes = 0;
    for (int e = 0; e < n_entries; ++e)
    {
        const auto& en = entries[e];
        const auto& d = en.data;
        if (d.elem_size < 1 || d.levels < 1) throw invalid("bad unstructured data descriptor");
        if (en.field_slot < 0 || en.buffer_slot < 0) throw invalid("negative slot");
        if (en.n_lids < 0 || (en.n_lids > 0 && !en.lids)) throw invalid("bad index list");
        max_field_slot = std::max(max_field_slot, en.field_slot);
        max_buf_slot = std::max(max_buf_slot, en.buffer_slot);
        if (en.n_lids == 0) continue;
        const int64_t elem = d.elem_size;
        bool wide = false;
        for (int64_t i = 0; i < en.n_lids; ++i)
        {
            if (en.lids[i] < 0) throw invalid("negative local index");
            if (en.lids[i] >= (int64_t(1) << 31)) wide = true;
        }
        int mode;
        int64_t L;
        if (d.levels == 1 || (d.levels_first && d.level_stride == 1))
        {
            mode = 0;  // one row per index: all levels contiguous on both sides
            L = d.levels * elem;
        }
        else
        {
            mode = d.levels_first ? 1 : 2;  // rows (i, l) i-major / rows (l, i) l-major
            L = elem;
        }
        // one segment of index range [a, a + n) of the list (mode 2 split: one level `lev`, as
        // a mode-0 segment of elem-byte rows at field offset lev * level stride)
        auto add = [&](int64_t a, int64_t n, int m, int64_t lev, uint64_t buf_off) {
            seg_u s{};  // slots: set per launch group below
            s.buf_off = buf_off;
            s.n = uint32_t(n);
            s.index_stride_b = d.index_stride * elem;
            s.level_stride_b = d.level_stride * elem;
            s.field_off = lev >= 0 ? lev * s.level_stride_b : 0;
            s.lid64 = wide ? 1 : 0;
            s.mode = uint8_t(m);
            const int64_t Ls = m == 0 && lev < 0 ? L : elem;
            if (m == 1)
            {
                s.row_levels = uint32_t(d.levels);
                s.mag_inner = make_magic(uint32_t(d.levels));
            }
            else if (m == 2)
                s.mag_inner = make_magic(uint32_t(n));
            const int64_t seg_bytes = n * (m == 0 ? Ls : int64_t(d.levels) * elem);
            s.row_bytes = uint32_t(Ls);
            s.bytes = uint32_t(seg_bytes);
            s.mag_row = make_magic(uint32_t(Ls));
            int w = wlog2_of(uint64_t(Ls));
            w = std::min(w, wlog2_of(s.buf_off));
            w = std::min(w, wlog2_of(uint64_t(s.field_off < 0 ? -s.field_off : s.field_off)));
            if (n > 1) w = std::min(w, wlog2_of(uint64_t(s.index_stride_b < 0 ? -s.index_stride_b : s.index_stride_b)));
            if (m != 0) w = std::min(w, wlog2_of(uint64_t(s.level_stride_b < 0 ? -s.level_stride_b : s.level_stride_b)));
            s.wlog2 = uint8_t(w);
            // 4/8-B rows whose consecutive lids are adjacent in the field (index stride = row
            // length): 16-B lane chunks, one field access per run of 16/L lids (copy_runs)
            s.runs = (g_tune.urun && m == 0 && (Ls == 4 || Ls == 8) && s.index_stride_b == Ls &&
                      s.buf_off % 16 == 0) ? 1 : 0;
            if (s.runs)
            {
                // run-heavy: at least half of the 16-B chunks hold 16/L consecutive lids
                const int64_t K = 16 / Ls, chunks = n / K;
                const int64_t* li = en.lids + a;
                int64_t hits = 0;
                for (int64_t c = 0; c < chunks; ++c)
                {
                    bool run = true;
                    for (int64_t j = 1; j < K && run; ++j) run = li[c * K + j] == li[c * K] + j;
                    hits += run ? 1 : 0;
                }
                if (chunks > 0 && 2 * hits >= chunks) s.runs = 2;
            }
            // index lists shared by the segments that read the same range (split levels)
            const auto key = std::make_pair(en.lids + a, n);
            auto it = lid_off.find(key);
            size_t off;
            if (it != lid_off.end()) off = it->second;
            else
            {
                lid_bytes = (lid_bytes + 15) & ~size_t(15);
                off = lid_bytes;
                lid_bytes += size_t(n) * (wide ? 8 : 4);
                lid_off.emplace(key, off);
                uploads.push_back({en.lids + a, n, wide, off});
            }
            pend.push_back({segs.size(), off});
            segs.push_back(s);
            gf.push_back(en.field_slot);
            gb.push_back(en.buffer_slot);
        };
        // a segment addresses its bytes with 32-bit offsets: lists of more than kSegLimit bytes
        // are planned as several segments (index ranges; a levels-last list level by level)
        constexpr int64_t kSegLimit = int64_t(1) << 30;
        const int64_t per_index = int64_t(d.levels) * elem;
        const int64_t total = en.n_lids * per_index;
        if (per_index > kSegLimit) throw invalid("unstructured row of more than 1 GiB");
        if (total <= kSegLimit && en.n_lids < (int64_t(1) << 32))
            add(0, en.n_lids, mode, -1, en.buffer_offset);
        else if (mode != 2)
        {
            const int64_t step = kSegLimit / per_index;
            for (int64_t a = 0; a < en.n_lids; a += step)
                add(a, std::min(step, en.n_lids - a), mode, -1,
                    en.buffer_offset + uint64_t(a * per_index));
        }
        else
        {
            const int64_t step = kSegLimit / elem;
            for (int64_t lev = 0; lev < d.levels; ++lev)
                for (int64_t a = 0; a < en.n_lids; a += step)
                    add(a, std::min(step, en.n_lids - a), 0, lev,
                        en.buffer_offset + uint64_t((lev * en.n_lids + a) * elem));
        }
        bytes += uint64_t(total);
    }
    n_segments = int32_t(segs.size());
    if (!segs.empty() && have_device())
    {
        std::vector<unsigned char> host(lid_bytes);
        for (auto& p : uploads)
        {
            if (p.wide)
            {
                int64_t* dst = reinterpret_cast<int64_t*>(host.data() + p.off);
                for (int64_t i = 0; i < p.n; ++i) dst[i] = p.lids[i];
            }
            else
            {
                int32_t* dst = reinterpret_cast<int32_t*>(host.data() + p.off);
                for (int64_t i = 0; i < p.n; ++i) dst[i] = int32_t(p.lids[i]);
            }
        }
        if (hipMalloc(&lid_store.lids, lid_bytes) != hipSuccess) throw hip_error("hipMalloc(lids)");
        if (hipMemcpy(lid_store.lids, host.data(), lid_bytes, hipMemcpyHostToDevice) != hipSuccess)
            throw hip_error("hipMemcpy(lids)");
        for (auto& p : pend) segs[p.seg].lids = static_cast<char*>(lid_store.lids) + p.off;
    }
    groups = build_groups(segs, gf, gb, direction);
}

int uplan::execute(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const
{
    return execute_groups(*this, &parity, fptr, nf, bptr, nb, [&](const kargs& a, const launch_group<seg_u>& grp) {
        // the run-path kernel when every segment qualifies with these pointers: flagged by the
        // planner, whole 16-B chunks per tile, 16-B aligned buffer ranges (both copies of a
        // double-buffered one), field base aligned to L
        bool runs = !grp.host_segs.empty();
        for (const seg_u& s : grp.host_segs)
            runs = runs && s.runs && s.tile_bytes % 16 == 0 &&
                   (a.buf_ptr[s.buf_slot] + s.buf_off) % 16 == 0 && a.dbl_off[s.buf_slot] % 16 == 0 &&
                   a.field_ptr[s.field_slot] % s.row_bytes == 0;
        return launch_unstructured(a, direction, stream, grid_for_tiles(a.n_tiles), runs);
    });
}

// ---------------------------------------------------------------------------------------------
// index-list put
// ---------------------------------------------------------------------------------------------
uput_plan::uput_plan(const ghx_uput_entry* src, const ghx_uput_entry* dst, int n_entries,
                     const ubuf_place* buf)
{
    auto mag = [](int64_t v) { return uint64_t(v < 0 ? -v : v); };
    // both sides' index lists in one device allocation: int32 where a list fits, per list
    struct lid_upload
    {
        const int64_t* lids;
        int64_t n;
        bool wide;
        size_t off;
    };
    std::vector<lid_upload> uploads;
    std::map<std::pair<const int64_t*, int64_t>, size_t> lid_off;  // -> index into uploads
    std::vector<std::pair<size_t, size_t>> pend;                   // per segment: src / dst upload
    size_t lid_bytes = 0;
    auto wide_list = [](const ghx_uput_entry& en) {
        bool wide = false;
        for (int64_t i = 0; i < en.n_lids; ++i)
        {
            if (en.lids[i] < 0) throw invalid("negative local index");
            if (en.lids[i] >= (int64_t(1) << 31)) wide = true;
        }
        return wide;
    };
    auto table = [&](const int64_t* lids, int64_t n, bool wide) {
        const auto key = std::make_pair(lids, n);
        auto it = lid_off.find(key);
        if (it != lid_off.end() && uploads[it->second].wide == wide) return it->second;
        lid_bytes = (lid_bytes + 15) & ~size_t(15);
        uploads.push_back({lids, n, wide, lid_bytes});
        lid_bytes += size_t(n) * (wide ? 8 : 4);
        lid_off[key] = uploads.size() - 1;
        return uploads.size() - 1;
    };
    // at least half of the list's 16-B chunks hold 16/L consecutive lids
    auto run_heavy = [](const int64_t* li, int64_t n, int64_t L) {
        const int64_t K = 16 / L, chunks = n / K;
        int64_t hits = 0;
        for (int64_t c = 0; c < chunks; ++c)
        {
            bool run = true;
            for (int64_t j = 1; j < K && run; ++j) run = li[c * K + j] == li[c * K] + j;
            hits += run ? 1 : 0;
        }
        return chunks > 0 && 2 * hits >= chunks;
    };
    for (int e = 0; e < n_entries; ++e)
    {
        const ghx_uput_entry &se = src[e], &de = dst[e];
        const ghx_udata_desc &sd = se.data, &dd = de.data;
        if (sd.elem_size < 1 || sd.levels < 1 || dd.elem_size < 1 || dd.levels < 1)
            throw invalid("bad unstructured data descriptor");
        if (se.field_slot < 0 || de.field_slot < 0) throw invalid("negative slot");
        if (se.field_slot >= GHX_MAX_SLOTS || de.field_slot >= GHX_MAX_SLOTS)
            throw invalid("a put plan takes at most 64 source and 64 target fields (one launch)");
        if (se.n_lids < 0 || de.n_lids < 0 || (se.n_lids > 0 && !se.lids) || (de.n_lids > 0 && !de.lids))
            throw invalid("bad index list");
        if (se.n_lids != de.n_lids || sd.elem_size != dd.elem_size || sd.levels != dd.levels ||
            (sd.levels_first != 0) != (dd.levels_first != 0))
            throw invalid("source and target index lists do not describe the same message bytes "
                          "(list lengths, element sizes, levels or level order differ)");
        max_src_slot = std::max(max_src_slot, se.field_slot);
        max_dst_slot = std::max(max_dst_slot, de.field_slot);
        if (buf) max_buf_slot = std::max(max_buf_slot, buf[e].slot);
        const bool swide = wide_list(se), dwide = wide_list(de);
        const int64_t elem = sd.elem_size;
        const int64_t per_index = int64_t(sd.levels) * elem;
        constexpr int64_t kSegLimit = int64_t(1) << 30;
        if (per_index > kSegLimit) throw invalid("unstructured row of more than 1 GiB");
        if (se.n_lids == 0) continue;
        // uplan's rule for both sides together: whole-index rows only where the levels are
        // contiguous on both
        const bool contiguous = sd.levels == 1 ||
                                (sd.levels_first && sd.level_stride == 1 && dd.level_stride == 1);
        const int mode = contiguous ? 0 : sd.levels_first ? 1 : 2;
        // one segment of index range [a, a + n) of both lists (mode 2 split: one level `lev`, as a
        // mode-0 segment of elem-byte rows at each side's field offset lev * level stride)
        auto add = [&](int64_t a, int64_t n, int m, int64_t lev) {
            seg_up s{};
            s.n = uint32_t(n);
            s.src_index_stride_b = sd.index_stride * elem;
            s.src_level_stride_b = sd.level_stride * elem;
            s.dst_index_stride_b = dd.index_stride * elem;
            s.dst_level_stride_b = dd.level_stride * elem;
            s.src_field_off = lev >= 0 ? lev * s.src_level_stride_b : 0;
            s.dst_field_off = lev >= 0 ? lev * s.dst_level_stride_b : 0;
            s.src_lid64 = swide ? 1 : 0;
            s.dst_lid64 = dwide ? 1 : 0;
            s.src_slot = uint16_t(se.field_slot);
            s.dst_slot = uint16_t(de.field_slot);
            s.mode = uint8_t(m);
            const int64_t Ls = m == 0 && lev < 0 ? per_index : elem;
            if (m == 1)
            {
                s.row_levels = uint32_t(sd.levels);
                s.mag_inner = make_magic(uint32_t(sd.levels));
            }
            else if (m == 2)
                s.mag_inner = make_magic(uint32_t(n));
            s.row_bytes = uint32_t(Ls);
            s.bytes = uint32_t(n * (m == 0 ? Ls : per_index));
            s.mag_row = make_magic(uint32_t(Ls));
            int w = wlog2_of(uint64_t(Ls));
            w = std::min(w, wlog2_of(mag(s.src_field_off)));
            w = std::min(w, wlog2_of(mag(s.dst_field_off)));
            if (n > 1)
            {
                w = std::min(w, wlog2_of(mag(s.src_index_stride_b)));
                w = std::min(w, wlog2_of(mag(s.dst_index_stride_b)));
            }
            if (m != 0)
            {
                w = std::min(w, wlog2_of(mag(s.src_level_stride_b)));
                w = std::min(w, wlog2_of(mag(s.dst_level_stride_b)));
            }
            if (buf)
            {
                // the segment's first message row in the send buffer, where uplan's pack puts it
                s.buf_slot = uint16_t(buf[e].slot);
                s.buf_off = buf[e].off + uint64_t(lev >= 0 ? (lev * se.n_lids + a) * elem : a * per_index);
                w = std::min(w, wlog2_of(s.buf_off));
            }
            s.wlog2 = uint8_t(w);
            const bool chunked = g_tune.urun && m == 0 && (Ls == 4 || Ls == 8);
            if (chunked && s.src_index_stride_b == Ls) s.src_runs = run_heavy(se.lids + a, n, Ls) ? 2 : 1;
            if (chunked && s.dst_index_stride_b == Ls) s.dst_runs = run_heavy(de.lids + a, n, Ls) ? 2 : 1;
            pend.emplace_back(table(se.lids + a, n, swide), table(de.lids + a, n, dwide));
            segs.push_back(s);
            message.push_back(e);
            first.push_back(a);
        };
        const int64_t total = se.n_lids * per_index;
        if (total <= kSegLimit && se.n_lids < (int64_t(1) << 32))
            add(0, se.n_lids, mode, -1);
        else if (mode != 2)
        {
            const int64_t step = kSegLimit / per_index;
            for (int64_t a = 0; a < se.n_lids; a += step) add(a, std::min(step, se.n_lids - a), mode, -1);
        }
        else
        {
            const int64_t step = kSegLimit / elem;
            for (int64_t lev = 0; lev < sd.levels; ++lev)
                for (int64_t a = 0; a < se.n_lids; a += step) add(a, std::min(step, se.n_lids - a), 0, lev);
        }
        bytes += uint64_t(total);
    }
    // tiles by the index-list rule (build_tiles / short_tile_rows / long_tile_bytes of seg_u):
    // whole rows; short rows by row count (run-heavy lists of either side: u_run_tile_rows)
    run_ok = g_tune.urun != 0 && !segs.empty();
    for (seg_up& s : segs)
    {
        uint32_t tb;
        if (s.row_bytes < g_tune.small_row_bytes)
        {
            const uint32_t rows = s.src_runs == 2 || s.dst_runs == 2 ? g_tune.u_run_tile_rows : g_tune.u_tile_rows;
            const uint64_t want = uint64_t(rows) * s.row_bytes;
            tb = uint32_t(std::max<uint64_t>(s.row_bytes, std::min<uint64_t>(want, kMaxTileBytes)));
        }
        else
            tb = std::max<uint32_t>(g_tune.u_tile_bytes, s.row_bytes);
        s.tile_bytes = tb - tb % s.row_bytes;
        run_ok = run_ok && s.mode == 0 && (s.row_bytes == 4 || s.row_bytes == 8) && s.tile_bytes % 16 == 0;
    }
    if (!segs.empty() && have_device())
    {
        std::vector<unsigned char> host(lid_bytes);
        for (const lid_upload& p : uploads)
        {
            if (p.wide)
            {
                int64_t* to = reinterpret_cast<int64_t*>(host.data() + p.off);
                for (int64_t i = 0; i < p.n; ++i) to[i] = p.lids[i];
            }
            else
            {
                int32_t* to = reinterpret_cast<int32_t*>(host.data() + p.off);
                for (int64_t i = 0; i < p.n; ++i) to[i] = int32_t(p.lids[i]);
            }
        }
        if (hipMalloc(&dev.lids, lid_bytes) != hipSuccess) throw hip_error("hipMalloc(put lids)");
        if (hipMemcpy(dev.lids, host.data(), lid_bytes, hipMemcpyHostToDevice) != hipSuccess)
            throw hip_error("hipMemcpy(put lids)");
        for (size_t k = 0; k < segs.size(); ++k)
        {
            segs[k].src_lids = static_cast<char*>(dev.lids) + uploads[pend[k].first].off;
            segs[k].dst_lids = static_cast<char*>(dev.lids) + uploads[pend[k].second].off;
        }
    }
    // one record per tile; short-row segments first (g_tune.order, as build_tiles)
    std::vector<size_t> idx(segs.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    if (g_tune.order == 1)
        std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
            return (segs[a].row_bytes < g_tune.small_row_bytes) > (segs[b].row_bytes < g_tune.small_row_bytes);
        });
    for (size_t i : idx)
    {
        const uint32_t nt = tiles_of(segs[i].bytes, segs[i].tile_bytes);
        for (uint32_t t = 0; t < nt; ++t)
        {
            recs.push_back(segs[i]);
            recs.back().first_tile = t;
        }
    }
    if (!recs.empty() && have_device())
    {
        const size_t rb = recs.size() * sizeof(seg_up);
        if (hipMalloc(&dev.recs, rb) != hipSuccess) throw hip_error("hipMalloc(put tile records)");
        if (hipMemcpy(dev.recs, recs.data(), rb, hipMemcpyHostToDevice) != hipSuccess)
            throw hip_error("hipMemcpy(put tile records)");
    }
}

int uput_plan::execute(void* const* src, int ns, void* const* dst, int nd, void* stream) const
{
    if (recs.empty()) return GHX_OK;
    if (!src || !dst || ns <= max_src_slot || nd <= max_dst_slot)
        throw invalid("pointer arrays do not cover the plan's slots");
    if (!dev.recs || !dev.lids) throw hip_error("plan has no device tables (no HIP device at creation)");
    kargs a{};
    a.tile_recs = dev.recs;
    a.n_tiles = uint32_t(recs.size());
    fill_slots(a.field_ptr, src, {}, max_src_slot + 1, "source field");
    fill_slots(a.buf_ptr, dst, {}, max_dst_slot + 1, "target field");
    // the run-path kernel when every segment qualifies with these pointers (both aligned to the row)
    bool runs = run_ok;
    for (size_t k = 0; runs && k < segs.size(); ++k)
        runs = a.field_ptr[segs[k].src_slot] % segs[k].row_bytes == 0 &&
               a.buf_ptr[segs[k].dst_slot] % segs[k].row_bytes == 0;
    return launch_put_u(a, stream, grid_for_tiles(a.n_tiles), runs);
}

// ---------------------------------------------------------------------------------------------
// fused index-list self exchange
// ---------------------------------------------------------------------------------------------
int uput_plan::execute_self(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const
{
    const uint32_t n_peer_tiles = uint32_t(peer_recs.size());
    if (recs.empty() && n_peer_tiles == 0) return GHX_OK;
    const int nfs = std::max(std::max(max_src_slot, max_dst_slot), peers ? peers->max_field_slot : -1);
    if (!fptr || !bptr || nf <= nfs || nb <= max_buf_slot)
        throw invalid("pointer arrays do not cover the plan's slots");
    if ((!recs.empty() && (!dev.recs || !dev.lids)) || (n_peer_tiles && !peer_dev.recs))
        throw hip_error("plan has no device tables (no HIP device at creation)");
    uint64_t field_ptr[GHX_MAX_SLOTS] = {}, buf_ptr[GHX_MAX_SLOTS] = {};
    fill_slots(field_ptr, fptr, {}, nfs + 1, "field");
    fill_slots(buf_ptr, bptr, {}, max_buf_slot + 1, "buffer");
    // the run-path kernel when every segment qualifies with these pointers: both fields aligned
    // to the row, every message chunk of the buffer 16-B aligned
    bool runs = run_ok;
    for (size_t k = 0; runs && k < segs.size(); ++k)
        runs = field_ptr[segs[k].src_slot] % segs[k].row_bytes == 0 &&
               field_ptr[segs[k].dst_slot] % segs[k].row_bytes == 0 &&
               (buf_ptr[segs[k].buf_slot] + segs[k].buf_off) % 16 == 0;
    if (!peers)
    {
        kargs a{};
        a.tile_recs = dev.recs;
        a.n_tiles = uint32_t(recs.size());
        std::copy(field_ptr, field_ptr + GHX_MAX_SLOTS, a.field_ptr);
        std::copy(buf_ptr, buf_ptr + GHX_MAX_SLOTS, a.buf_ptr);
        return launch_self_u(a, stream, grid_for_tiles(a.n_tiles), runs);
    }
    // the mixed form: the run variant only when the peer part qualifies too (uplan::execute's rule)
    for (const seg_u& s : peers->groups[0].host_segs)
        runs = runs && s.runs && s.tile_bytes % 16 == 0 && (buf_ptr[s.buf_slot] + s.buf_off) % 16 == 0 &&
               field_ptr[s.field_slot] % s.row_bytes == 0;
    kargs_um a{};
    a.self_recs = dev.recs;
    a.peer_recs = peer_dev.recs;
    a.n_self_tiles = uint32_t(recs.size());
    a.n_peer_tiles = n_peer_tiles;
    std::copy(field_ptr, field_ptr + GHX_MAX_SLOTS, a.field_ptr);
    std::copy(buf_ptr, buf_ptr + GHX_MAX_SLOTS, a.buf_ptr);
    return launch_pack_self_u(a, stream, grid_for_tiles(a.n_self_tiles + a.n_peer_tiles), runs);
}

namespace
{
// make_uself and make_umixed: the self messages' plan and every check that makes ONE launch equal
// pack followed by unpack; with `peers`, the messages that leave the rank (packed by the same
// launch) join the buffer-range check and the cell check.
std::unique_ptr<uput_plan> plan_uself(const ghx_upack_entry* src, const ghx_upack_entry* dst, int n,
                                      const ghx_upack_entry* peers, int n_peers)
{
    const size_t nk = n > 0 ? size_t(n) : 0;
    std::vector<ghx_uput_entry> se(nk), de(nk);
    std::vector<ubuf_place> place(nk);
    for (int k = 0; k < n; ++k)
    {
        const ghx_upack_entry &s = src[k], &d = dst[k];
        if (s.field_slot < 0 || d.field_slot < 0 || s.buffer_slot < 0 || d.buffer_slot < 0)
            throw invalid("negative slot");
        if (s.field_slot >= GHX_MAX_SLOTS || d.field_slot >= GHX_MAX_SLOTS || s.buffer_slot >= GHX_MAX_SLOTS)
            throw invalid("a fused index-list self exchange takes at most 64 field and 64 buffer "
                          "slots (one launch, no launch groups)");
        if (s.buffer_slot != d.buffer_slot || s.buffer_offset != d.buffer_offset)
            throw invalid("the pack and the unpack entry of a message differ in buffer slot or "
                          "buffer offset (they do not name the same buffer bytes)");
        se[size_t(k)] = {s.data, s.field_slot, s.lids, s.n_lids};
        de[size_t(k)] = {d.data, d.field_slot, d.lids, d.n_lids};
        place[size_t(k)] = {s.buffer_slot, s.buffer_offset};
    }
    for (int j = 0; j < n_peers; ++j)
    {
        if (peers[j].field_slot < 0 || peers[j].buffer_slot < 0) throw invalid("negative slot");
        if (peers[j].field_slot >= GHX_MAX_SLOTS || peers[j].buffer_slot >= GHX_MAX_SLOTS)
            throw invalid("a peer message's field or buffer slot is 64 or more (the pack with self "
                          "messages is one launch, no launch groups)");
    }
    // descriptors, lids and the agreement of the two sides: the put's checks
    auto p = std::make_unique<uput_plan>(se.data(), de.data(), n, place.data());
    // the peer messages: descriptors and lids by the pack plan's checks, its segments and tiles
    if (peers)
    {
        p->peers = std::make_unique<uplan>(peers, n_peers, 0);
        p->max_buf_slot = std::max(p->max_buf_slot, p->peers->max_buf_slot);
        const launch_group<seg_u>& g = p->peers->groups[0];  // slots < 64: one group, identity maps
        for (size_t t = 0; t < g.n_tiles; ++t)
        {
            p->peer_recs.push_back(g.host_segs[g.host_tiles[2 * t]]);
            p->peer_recs.back().first_tile = g.host_tiles[2 * t + 1];
        }
        if (!p->peer_recs.empty() && have_device())
        {
            const size_t rb = p->peer_recs.size() * sizeof(seg_u);
            if (hipMalloc(&p->peer_dev.recs, rb) != hipSuccess) throw hip_error("hipMalloc(peer tile records)");
            if (hipMemcpy(p->peer_dev.recs, p->peer_recs.data(), rb, hipMemcpyHostToDevice) != hipSuccess)
                throw hip_error("hipMemcpy(peer tile records)");
        }
    }
    // no two messages share buffer bytes
    struct range
    {
        int32_t slot;
        uint64_t first, end;
        bool peer;
    };
    std::vector<range> ranges;
    auto add_range = [&](const ghx_upack_entry& e, bool peer) {
        const uint64_t nb = uint64_t(e.n_lids) * uint64_t(e.data.levels) * uint64_t(e.data.elem_size);
        if (nb) ranges.push_back({e.buffer_slot, e.buffer_offset, e.buffer_offset + nb, peer});
    };
    for (int k = 0; k < n; ++k) add_range(src[k], false);
    for (int j = 0; j < n_peers; ++j) add_range(peers[j], true);
    std::sort(ranges.begin(), ranges.end(), [](const range& a, const range& b) {
        return std::make_pair(a.slot, a.first) < std::make_pair(b.slot, b.first);
    });
    for (size_t i = 1; i < ranges.size(); ++i)
        if (ranges[i].slot == ranges[i - 1].slot && ranges[i].first < ranges[i - 1].end)
            throw invalid(ranges[i].peer || ranges[i - 1].peer
                              ? "a peer message overlaps another message in one buffer"
                              : "two messages overlap in one buffer");
    // A fused launch reads and writes in no defined order: it equals pack followed by unpack only
    // if no cell (field slot, lid) is read and written, and none is written twice.
    std::vector<std::pair<int32_t, int64_t>> reads, writes;
    for (int k = 0; k < n; ++k)
        for (int64_t i = 0; i < src[k].n_lids; ++i)
        {
            reads.emplace_back(src[k].field_slot, src[k].lids[i]);
            writes.emplace_back(dst[k].field_slot, dst[k].lids[i]);
        }
    std::sort(writes.begin(), writes.end());
    if (std::adjacent_find(writes.begin(), writes.end()) != writes.end())
        throw invalid("a target cell of a field slot appears twice (the launch's stores have no order)");
    for (const auto& c : reads)
        if (std::binary_search(writes.begin(), writes.end(), c))
            throw invalid("a cell of a field slot is both a source and a target of the plan (the "
                          "launch's loads and stores have no order)");
    // the hazard rule of the mixed form: in the two-launch path every pack load precedes every
    // unpack store; here a peer tile may load a cell after a self tile has stored it
    for (int j = 0; j < n_peers; ++j)
        for (int64_t i = 0; i < peers[j].n_lids; ++i)
            if (std::binary_search(writes.begin(), writes.end(), std::make_pair(peers[j].field_slot, peers[j].lids[i])))
                throw invalid("a target cell of a self message is a source cell of a peer message "
                              "(the launch's loads and stores have no order)");
    return p;
}
}  // namespace

std::unique_ptr<uput_plan> make_uself(const ghx_upack_entry* src, const ghx_upack_entry* dst, int n)
{
    return plan_uself(src, dst, n, nullptr, 0);
}

std::unique_ptr<uput_plan> make_umixed(const ghx_upack_entry* src, const ghx_upack_entry* dst, int n_self,
                                       const ghx_upack_entry* peers, int n_peers)
{
    if (n_self < 1 || !src || !dst)
        throw invalid("no self message (an exchange of peer messages alone is ghx_uplan_create's)");
    if (n_peers < 1 || !peers)
        throw invalid("no peer message (an exchange of self messages alone is ghx_uself_create's)");
    return plan_uself(src, dst, n_self, peers, n_peers);
}

}  // namespace ghx
