// ghx_accum_plan.cpp — the planner of the adjoint accumulate (uaccum_plan, k_accum_u and its get
// form k_accum_get_u): the inverted index from destination cells to their contributions, built on
// the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ghx_plan.hpp"

namespace ghx
{
namespace
{
bool have_device()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

int dtype_size(int32_t dt)
{
    switch (dt)
    {
        case GHX_DT_F32:
        case GHX_DT_I32: return 4;
        case GHX_DT_F64:
        case GHX_DT_I64: return 8;
        default: return 0;
    }
}

bool same_desc(const ghx_udata_desc& a, const ghx_udata_desc& b)
{
    return a.elem_size == b.elem_size && a.levels == b.levels && (a.levels_first != 0) == (b.levels_first != 0) &&
           a.index_stride == b.index_stride && a.level_stride == b.level_stride;
}

template<typename T>
void to_device(void*& to, const std::vector<T>& from, const char* what)
{
    if (from.empty()) return;
    const size_t nb = from.size() * sizeof(T);
    if (hipMalloc(&to, nb) != hipSuccess) throw hip_error(std::string("hipMalloc(") + what + ")");
    if (hipMemcpy(to, from.data(), nb, hipMemcpyHostToDevice) != hipSuccess)
        throw hip_error(std::string("hipMemcpy(") + what + ")");
}

constexpr uint64_t kMaxRecords = 0xffffffffull;  // record and destination indices are 32-bit
}  // namespace

uaccum_plan::tables::~tables()
{
    for (void* p : {tiles, ranges, lids, contribs, entries})
        if (p) (void)hipFree(p);
}

namespace
{
std::string cell_name(const std::pair<int32_t, int64_t>& c)
{
    return "(field slot " + std::to_string(c.first) + ", lid " + std::to_string(c.second) + ")";
}
using cell_list = std::vector<std::pair<int32_t, int64_t>>;
// the first cell two sorted lists share, or null
const std::pair<int32_t, int64_t>* first_common(const cell_list& a, const cell_list& b)
{
    for (size_t i = 0, k = 0; i < a.size() && k < b.size();)
    {
        if (a[i] == b[k]) return &a[i];
        if (a[i] < b[k]) ++i;
        else ++k;
    }
    return nullptr;
}
}  // namespace

uaccum_plan::uaccum_plan(const ghx_upack_entry* contrib, const int32_t* dtypes, int n,
                         const ghx_upack_entry* zero, int n_zero, const ghx_upack_entry* const* source)
    : get(source != nullptr)
{
    // per field slot: the descriptor and dtype every entry of the slot must share
    const ghx_udata_desc* slot_desc[GHX_MAX_SLOTS] = {};
    int32_t slot_dtype[GHX_MAX_SLOTS] = {};
    uint64_t n_records = 0, n_zero_cells = 0;
    // is_zero: the buffer members play no part (a zero entry, a source, an entry with a source)
    auto check_entry = [&](const ghx_upack_entry& en, bool is_zero) {
        const ghx_udata_desc& d = en.data;
        if (d.levels < 1) throw invalid("bad unstructured data descriptor (levels < 1)");
        if (en.field_slot < 0 || (!is_zero && en.buffer_slot < 0)) throw invalid("negative slot");
        if (en.field_slot >= GHX_MAX_SLOTS || (!is_zero && en.buffer_slot >= GHX_MAX_SLOTS))
            throw invalid("an accumulate plan takes at most 64 field and 64 buffer slots (one launch)");
        if (en.n_lids < 0 || (en.n_lids > 0 && !en.lids)) throw invalid("bad index list");
        const ghx_udata_desc*& known = slot_desc[en.field_slot];
        if (known && !same_desc(*known, d))
            throw invalid("two entries of field slot " + std::to_string(en.field_slot) +
                          " differ in their data descriptor");
        known = &d;
        slot_elem[en.field_slot] = uint8_t(d.elem_size);
        max_field_slot = std::max(max_field_slot, en.field_slot);
    };
    for (int e = 0; e < n; ++e)
    {
        const ghx_upack_entry& en = contrib[e];
        const int sz = dtype_size(dtypes[e]);
        if (!sz) throw invalid("unknown dtype code " + std::to_string(dtypes[e]) + " (GHX_DT_F32, _F64, _I32, _I64)");
        if (sz != en.data.elem_size)
            throw invalid("dtype code " + std::to_string(dtypes[e]) + " has " + std::to_string(sz) +
                          " bytes, the entry's elem_size is " + std::to_string(en.data.elem_size));
        const ghx_upack_entry* src = source ? source[e] : nullptr;
        check_entry(en, src != nullptr);
        int32_t& dt = slot_dtype[en.field_slot];
        if (dt && dt != dtypes[e])
            throw invalid("two entries of field slot " + std::to_string(en.field_slot) + " differ in their dtype");
        dt = dtypes[e];
        n_records += uint64_t(en.n_lids);
        if (src)
        {
            // the halo side of the same message: the same cells in the same order, whatever its layout
            if (src->n_lids != en.n_lids || src->data.levels != en.data.levels || src->data.elem_size != en.data.elem_size)
                throw invalid("contribution entry " + std::to_string(e) + " and its source differ in n_lids, levels or "
                              "elem_size (" + std::to_string(en.n_lids) + " / " + std::to_string(en.data.levels) + " / " +
                              std::to_string(en.data.elem_size) + " against " + std::to_string(src->n_lids) + " / " +
                              std::to_string(src->data.levels) + " / " + std::to_string(src->data.elem_size) + ")");
            check_entry(*src, true);
            int32_t& sdt = slot_dtype[src->field_slot];
            if (sdt && sdt != dtypes[e])
                throw invalid("two entries of field slot " + std::to_string(src->field_slot) + " differ in their dtype");
            sdt = dtypes[e];
            ++n_field_sources;
            continue;
        }
        if (en.buffer_offset % uint64_t(sz))
            throw invalid("buffer offset is not a multiple of the element size");
        max_buf_slot = std::max(max_buf_slot, en.buffer_slot);
        bytes += uint64_t(en.n_lids) * uint64_t(en.data.levels) * uint64_t(sz);
    }
    for (int k = 0; k < n_zero; ++k)
    {
        const ghx_upack_entry& en = zero[k];
        if (en.data.elem_size != 4 && en.data.elem_size != 8)
            throw invalid("a zero entry's elem_size is " + std::to_string(en.data.elem_size) +
                          ", not that of a dtype (4 or 8)");
        check_entry(en, true);
        n_zero_cells += uint64_t(en.n_lids);
    }
    // before any list is read: the tables index records and destinations with 32 bits
    if (n_records > kMaxRecords)
        throw invalid("more than 2^32 - 1 contribution records (" + std::to_string(n_records) + ")");
    if (n_zero_cells > kMaxRecords) throw invalid("more than 2^32 - 1 zero cells");

    // the inverted index: every (cell, entry, position), sorted
    struct item
    {
        int64_t lid;
        int32_t slot;
        uint32_t entry, pos;
    };
    std::vector<item> items;
    items.reserve(size_t(n_records));
    entries.resize(size_t(n));
    for (int e = 0; e < n; ++e)
    {
        const ghx_upack_entry& en = contrib[e];
        acc_entry& r = entries[size_t(e)];
        r.buf_off = en.buffer_offset;
        r.n = uint32_t(en.n_lids);
        r.levels = uint32_t(en.data.levels);
        r.levels_first = en.data.levels_first ? 1 : 0;
        r.buf_slot = uint32_t(en.buffer_slot);
        r.pos_stride = r.levels_first ? r.levels : 1;
        r.lev_stride = r.levels_first ? 1 : r.n;
        entry_elem.push_back(uint8_t(en.data.elem_size));
        if (get)
        {
            const ghx_upack_entry* src = source[e];
            acc_get_entry g{};
            g.base = src ? 0 : en.buffer_offset;
            g.at_stride = src ? src->data.index_stride : int64_t(r.pos_stride);
            g.lev_stride = src ? src->data.level_stride : int64_t(r.lev_stride);
            g.tab = src ? uint32_t(src->field_slot) : uint32_t(GHX_MAX_SLOTS + en.buffer_slot);
            g.field_src = src ? 1 : 0;
            get_entries.push_back(g);
        }
        for (int64_t i = 0; i < en.n_lids; ++i)
        {
            if (en.lids[i] < 0) throw invalid("negative local index");
            items.push_back({en.lids[i], en.field_slot, uint32_t(e), uint32_t(i)});
        }
    }
    std::sort(items.begin(), items.end(), [](const item& a, const item& b) {
        if (a.slot != b.slot) return a.slot < b.slot;
        if (a.lid != b.lid) return a.lid < b.lid;
        if (a.entry != b.entry) return a.entry < b.entry;
        return a.pos < b.pos;
    });
    contribs.resize(items.size());
    for (size_t j = 0; j < items.size(); ++j)
    {
        const item& it = items[j];
        if (j == 0 || items[j - 1].slot != it.slot || items[j - 1].lid != it.lid)
        {
            dest_slot.push_back(it.slot);
            dest_lid.push_back(it.lid);
            ranges.push_back({uint32_t(j), 0});
        }
        ++ranges.back().count;
        contribs[j] = {it.entry, it.pos};
    }
    n_dest = ranges.size();
    for (const acc_range& r : ranges) max_per_dest = std::max(max_per_dest, r.count);

    // a get plan: the source lid of every record of an entry with a source. One record reads a
    // source cell and nothing else touches it, or the in-lane zero would race
    cell_list sc;
    if (get)
    {
        src_lid.assign(items.size(), -1);
        for (size_t j = 0; j < items.size(); ++j)
        {
            const ghx_upack_entry* src = source[items[j].entry];
            if (!src) continue;
            const int64_t l = src->lids[items[j].pos];
            if (l < 0) throw invalid("negative local index");
            src_lid[j] = l;
            rec64 = rec64 || l >= (int64_t(1) << 31);
            sc.emplace_back(src->field_slot, l);
        }
        std::sort(sc.begin(), sc.end());
        const auto twice = std::adjacent_find(sc.begin(), sc.end());
        if (twice != sc.end())
            throw invalid("source cell " + cell_name(*twice) + " is read by more than one record (a lid repeated in a "
                          "receive list, or two receive lists of one field slot that name it): the second reader "
                          "would see the first one's zero");
        cell_list dc;
        for (size_t a = 0; a < size_t(n_dest); ++a) dc.emplace_back(dest_slot[a], dest_lid[a]);
        if (const auto* c = first_common(sc, dc))
            throw invalid("source cell " + cell_name(*c) + " is also a sum destination");
    }
    // a zero entry that is a contribution's source (same field slot, same list) gets no zero tile
    auto is_source = [&](const ghx_upack_entry& z) {
        for (int e = 0; get && e < n; ++e)
        {
            const ghx_upack_entry* src = source[e];
            if (src && src->field_slot == z.field_slot && src->n_lids == z.n_lids &&
                (src->lids == z.lids || z.n_lids == 0 ||
                 std::memcmp(src->lids, z.lids, size_t(z.n_lids) * sizeof(int64_t)) == 0))
                return true;
        }
        return false;
    };

    // the zero cells, distinct and sorted, none of them a sum destination
    cell_list zc;
    zc.reserve(size_t(n_zero_cells));
    for (int k = 0; k < n_zero; ++k)
    {
        for (int64_t i = 0; i < zero[k].n_lids; ++i)
            if (zero[k].lids[i] < 0) throw invalid("negative local index");
        if (is_source(zero[k])) continue;
        for (int64_t i = 0; i < zero[k].n_lids; ++i) zc.emplace_back(zero[k].field_slot, zero[k].lids[i]);
    }
    std::sort(zc.begin(), zc.end());
    zc.erase(std::unique(zc.begin(), zc.end()), zc.end());
    if (const auto* c = first_common(sc, zc))
        throw invalid("source cell " + cell_name(*c) + " lies in a zero entry that is no source (its zero tile would "
                      "race with the load)");
    for (size_t a = 0, b = 0; a < size_t(n_dest) && b < zc.size();)
    {
        const std::pair<int32_t, int64_t> s{dest_slot[a], dest_lid[a]};
        if (s == zc[b])
            throw invalid("cell (field slot " + std::to_string(s.first) + ", lid " + std::to_string(s.second) +
                          ") is both a sum destination and a zero destination");
        if (s < zc[b]) ++a;
        else ++b;
    }
    n_zero_dest = zc.size();
    for (const auto& c : zc)
    {
        dest_slot.push_back(c.first);
        dest_lid.push_back(c.second);
    }
    for (int64_t l : dest_lid) lid64 = lid64 || l >= (int64_t(1) << 31);

    // tiles: g_tune.u_tile_rows destination rows of one field slot (fewer where rows * levels
    // would not fit the lanes' 32-bit element index)
    auto add_tiles = [&](uint64_t first, uint64_t last, bool is_zero) {
        for (uint64_t a = first; a < last;)
        {
            const int32_t slot = dest_slot[size_t(a)];
            uint64_t b = a;
            while (b < last && dest_slot[size_t(b)] == slot) ++b;
            const ghx_udata_desc& d = *slot_desc[slot];
            const uint64_t rows = std::max<uint64_t>(1, std::min<uint64_t>(g_tune.u_tile_rows, 0x7fffffffu / uint32_t(d.levels)));
            for (; a < b; a += rows)
            {
                acc_tile t{};
                t.index_stride_b = d.index_stride * d.elem_size;
                t.level_stride_b = d.level_stride * d.elem_size;
                t.first_dest = uint32_t(a);
                t.n_rows = uint32_t(std::min(rows, b - a));
                t.levels = uint32_t(d.levels);
                t.lcontig = d.level_stride == 1 ? 1 : 0;
                t.mag = make_magic(t.lcontig ? t.levels : t.n_rows);
                t.field_slot = uint16_t(slot);
                t.zero = is_zero ? 1 : 0;
                t.dtype = uint8_t(is_zero ? (d.elem_size == 8 ? GHX_DT_I64 : GHX_DT_I32) : slot_dtype[slot]);
                tiles.push_back(t);
            }
            a = b;
        }
    };
    add_tiles(0, n_dest, false);
    n_sum_tiles = uint32_t(tiles.size());
    add_tiles(n_dest, n_dest + n_zero_dest, true);

    if (tiles.empty() || !have_device()) return;
    to_device(dev.tiles, tiles, "accumulate tiles");
    to_device(dev.ranges, ranges, "accumulate ranges");
    if (!get)
    {
        to_device(dev.contribs, contribs, "accumulate records");
        to_device(dev.entries, entries, "accumulate entries");
    }
    else
    {
        // the records with their source resolved: the position, or the source lid
        auto at = [&](size_t j) { return src_lid[j] < 0 ? uint64_t(contribs[j].pos) : uint64_t(src_lid[j]); };
        if (rec64)
        {
            std::vector<acc_get_rec64> recs(contribs.size());
            for (size_t j = 0; j < recs.size(); ++j) recs[j] = {contribs[j].entry, 0, at(j)};
            to_device(dev.contribs, recs, "get-accumulate records");
        }
        else
        {
            std::vector<acc_get_rec> recs(contribs.size());
            for (size_t j = 0; j < recs.size(); ++j) recs[j] = {contribs[j].entry, uint32_t(at(j))};
            to_device(dev.contribs, recs, "get-accumulate records");
        }
        to_device(dev.entries, get_entries, "get-accumulate entries");
    }
    if (lid64) to_device(dev.lids, dest_lid, "accumulate lids");
    else to_device(dev.lids, std::vector<int32_t>(dest_lid.begin(), dest_lid.end()), "accumulate lids");
}

int uaccum_plan::execute(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const
{
    if (get) throw invalid("a get plan (ghx_uaccum_get_create) is launched by ghx_uaccum_get_execute");
    const uint32_t n_tiles = zero_halos ? uint32_t(tiles.size()) : n_sum_tiles;
    if (n_tiles == 0) return GHX_OK;
    if (!fptr || !bptr || nf <= max_field_slot || nb <= max_buf_slot)
        throw invalid("pointer arrays do not cover the plan's slots");
    if (!dev.tiles || !dev.lids) throw hip_error("plan has no device tables (no HIP device at creation)");
    kargs_ua a{};
    a.tiles = static_cast<const acc_tile*>(dev.tiles);
    a.ranges = static_cast<const acc_range*>(dev.ranges);
    a.lids = dev.lids;
    a.contribs = static_cast<const acc_contrib*>(dev.contribs);
    a.entries = static_cast<const acc_entry*>(dev.entries);
    a.n_tiles = n_tiles;
    a.lid64 = lid64 ? 1 : 0;
    for (int s = 0; s <= max_field_slot; ++s)
    {
        if (!slot_elem[s]) continue;
        if (!fptr[s]) throw invalid("null field pointer");
        a.field_ptr[s] = reinterpret_cast<uint64_t>(fptr[s]);
        if (a.field_ptr[s] % slot_elem[s]) throw invalid("a field pointer is not aligned to its element");
    }
    for (size_t e = 0; e < entries.size(); ++e)
    {
        const uint32_t b = entries[e].buf_slot;
        if (!bptr[b]) throw invalid("null buffer pointer");
        a.buf_ptr[b] = reinterpret_cast<uint64_t>(bptr[b]);
        if (a.buf_ptr[b] % entry_elem[e]) throw invalid("a buffer pointer is not aligned to its elements");
    }
    return launch_accum_u(a, stream, grid_for_tiles(n_tiles));
}

int uaccum_plan::execute_get(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const
{
    if (!get) throw invalid("a plan of ghx_uaccum_create is launched by ghx_uaccum_execute");
    const uint32_t n_tiles = zero_halos ? uint32_t(tiles.size()) : n_sum_tiles;
    if (n_tiles == 0) return GHX_OK;
    // the buffers of the entries without a source alone
    if (!fptr || nf <= max_field_slot || nb <= max_buf_slot || (max_buf_slot >= 0 && !bptr))
        throw invalid("pointer arrays do not cover the plan's slots");
    if (!dev.tiles || !dev.lids) throw hip_error("plan has no device tables (no HIP device at creation)");
    kargs_uag a{};
    a.tiles = static_cast<const acc_tile*>(dev.tiles);
    a.ranges = static_cast<const acc_range*>(dev.ranges);
    a.lids = dev.lids;
    a.recs = dev.contribs;
    a.entries = static_cast<const acc_get_entry*>(dev.entries);
    a.n_tiles = n_tiles;
    a.lid64 = lid64 ? 1 : 0;
    a.rec64 = rec64 ? 1 : 0;
    a.zero_src = zero_halos ? 1 : 0;
    for (int s = 0; s <= max_field_slot; ++s)
    {
        if (!slot_elem[s]) continue;
        if (!fptr[s]) throw invalid("null field pointer");
        a.ptr[s] = reinterpret_cast<uint64_t>(fptr[s]);
        if (a.ptr[s] % slot_elem[s]) throw invalid("a field pointer is not aligned to its element");
    }
    for (size_t e = 0; e < get_entries.size(); ++e)
    {
        if (get_entries[e].field_src) continue;
        const uint32_t b = entries[e].buf_slot;
        if (!bptr[b]) throw invalid("null buffer pointer");
        a.ptr[GHX_MAX_SLOTS + b] = reinterpret_cast<uint64_t>(bptr[b]);
        if (a.ptr[GHX_MAX_SLOTS + b] % entry_elem[e]) throw invalid("a buffer pointer is not aligned to its elements");
    }
    return launch_accum_get_u(a, stream, grid_for_tiles(n_tiles));
}

}  // namespace ghx
