// ghx_saccum_plan.cpp — the planner of the structured adjoint accumulate (saccum_plan, k_accum_s):
// the arrangement of a field's overlapping contribution boxes into disjoint sub-boxes, each with
// one list of sources, built on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <map>
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

int wlog2_of(uint64_t v) { return v ? std::min(4, __builtin_ctzll(v)) : 4; }

template<typename T>
void to_device(void*& to, const std::vector<T>& from, const char* what)
{
    if (from.empty()) return;
    const size_t nb = from.size() * sizeof(T);
    if (hipMalloc(&to, nb) != hipSuccess) throw hip_error(std::string("hipMalloc(") + what + ")");
    if (hipMemcpy(to, from.data(), nb, hipMemcpyHostToDevice) != hipSuccess)
        throw hip_error(std::string("hipMemcpy(") + what + ")");
}

bool same_field(const ghx_field_desc& a, const ghx_field_desc& b)
{
    bool same = a.dim == b.dim && a.elem_size == b.elem_size && a.num_components == b.num_components &&
                (a.has_components != 0) == (b.has_components != 0);
    for (int d = 0; same && d < a.dim; ++d)
        same = a.layout[d] == b.layout[d] && a.byte_strides[d] == b.byte_strides[d] &&
               a.offsets[d] == b.offsets[d] && a.extents[d] == b.extents[d];
    return same;
}

// one box of an entry: its spatial bounds, where its dense buffer box starts and the buffer byte
// stride of every field dim in it (layout order, component axis included: ghx_plan.cpp,
// add_box_segments)
struct cbox
{
    uint32_t entry, box;
    int64_t first[GHX_MAX_DIM], last[GHX_MAX_DIM];
    int32_t buf_slot;
    uint64_t buf_off;
    uint64_t bstride[GHX_MAX_DIM];
    // a field source (get plan): buf_slot is the source field's slot, buf_off the field byte offset
    // of the source box's origin and bstride the source field's byte strides (a cubed-sphere space:
    // of the image of the box's first cell, and signed strides mod 2^64; neg: the components it negates)
    bool field_src;
    uint8_t neg;
};

struct slot_boxes
{
    const ghx_field_desc* desc = nullptr;
    int32_t dtype = 0;
    std::vector<cbox> sum, zero;
    std::vector<cbox> src;       // the source boxes that lie in this slot's field (get plan)
    std::vector<char> zero_is_src;  // per zero box: its entry is a contribution's source
};

bool meet(const cbox& a, const cbox& b, int spatial)
{
    bool m = true;
    for (int d = 0; m && d < spatial; ++d) m = a.first[d] <= b.last[d] && b.first[d] <= a.last[d];
    return m;
}

bool same_boxes(const ghx_pack_entry& a, const ghx_pack_entry& b)
{
    if (a.field_slot != b.field_slot || a.n_boxes != b.n_boxes) return false;
    const int spatial = a.field.dim - (a.field.has_components ? 1 : 0);
    for (int k = 0; k < a.n_boxes; ++k)
        for (int d = 0; d < spatial; ++d)
            if (a.boxes[k].first[d] != b.boxes[k].first[d] || a.boxes[k].last[d] != b.boxes[k].last[d]) return false;
    return true;
}

constexpr uint64_t kMaxRecords = 0xffffffffull;  // source and tile indices are 32-bit
}  // namespace

saccum_plan::tables::~tables()
{
    for (void* p : {tiles, srcs})
        if (p) (void)hipFree(p);
}

saccum_plan::saccum_plan(const ghx_pack_entry* contrib, const int32_t* dtypes, int n, const ghx_pack_entry* zero,
                         int n_zero, const ghx_pack_entry* const* source, const xseg* const* space)
    : get(source != nullptr), rotated(source != nullptr && space != nullptr)
{
    std::map<int32_t, slot_boxes> slots;
    enum { k_sum, k_zero, k_src };
    // kind k_sum with `paired`: the entry's contributions come from a source field, not its buffer
    auto add_entry = [&](const ghx_pack_entry& en, uint32_t e, int kind, bool paired = false) {
        const ghx_field_desc& f = en.field;
        const bool is_zero = kind == k_zero, buffered = kind == k_sum && !paired;
        validate_field(f);
        if (en.field_slot < 0 || (buffered && en.buffer_slot < 0)) throw invalid("negative slot");
        if (en.field_slot >= GHX_MAX_SLOTS || (buffered && en.buffer_slot >= GHX_MAX_SLOTS))
            throw invalid("an accumulate plan takes at most 64 field and 64 buffer slots (one launch)");
        if (en.n_boxes < 0 || (en.n_boxes > 0 && !en.boxes)) throw invalid("bad boxes");
        for (int d = 0; d < f.dim; ++d)
            if (f.byte_strides[d] % f.elem_size)
                throw invalid("a byte stride of the field is not a multiple of the element size");
        slot_boxes& sb = slots[en.field_slot];
        if (sb.desc && !same_field(*sb.desc, f))
            throw invalid("two entries of field slot " + std::to_string(en.field_slot) +
                          " differ in their field descriptor");
        sb.desc = &f;
        slot_elem[en.field_slot] = uint8_t(f.elem_size);
        max_field_slot = std::max(max_field_slot, en.field_slot);
        const int D = f.dim, spatial = D - (f.has_components ? 1 : 0);
        int by_speed[GHX_MAX_DIM];
        for (int d = 0; d < D; ++d) by_speed[D - 1 - f.layout[d]] = d;
        uint64_t off = en.buffer_offset;
        for (int b = 0; b < en.n_boxes; ++b)
        {
            cbox c{};
            c.entry = e;
            c.box = uint32_t(b);
            c.buf_slot = kind == k_src ? en.field_slot : en.buffer_slot;
            c.buf_off = off;
            c.field_src = kind == k_src;
            int64_t ext[GHX_MAX_DIM];
            for (int d = 0; d < D; ++d)
            {
                c.first[d] = d < spatial ? en.boxes[b].first[d] : 0;
                c.last[d] = d < spatial ? en.boxes[b].last[d] : f.num_components - 1;
                ext[d] = c.last[d] - c.first[d] + 1;
                if (ext[d] <= 0) throw invalid("iteration space: first must be <= last");
                // the rule of ghx_plan_create (add_box_segments)
                const int64_t o = d < spatial ? f.offsets[d] : 0;
                if (f.extents[d] > 0 && (c.first[d] + o < 0 || c.last[d] + o >= f.extents[d]))
                    throw invalid("iteration space outside the field extents");
            }
            uint64_t bs = uint64_t(f.elem_size);
            for (int k = 0; k < D; ++k)
            {
                c.bstride[by_speed[k]] = bs;
                bs *= uint64_t(ext[by_speed[k]]);
            }
            off += bs;
            if (kind == k_src)
            {
                // where the box lies in its field, in field bytes
                c.buf_off = 0;
                for (int d = 0; d < D; ++d)
                {
                    c.buf_off += uint64_t(c.first[d] + (d < spatial ? f.offsets[d] : 0)) * uint64_t(f.byte_strides[d]);
                    c.bstride[d] = uint64_t(f.byte_strides[d]);
                }
            }
            (kind == k_src ? sb.src : is_zero ? sb.zero : sb.sum).push_back(c);
        }
    };
    // contribution entry e reads box k of `src` where it would read box k of its buffer
    auto pair_entry = [&](const ghx_pack_entry& en, uint32_t e, const ghx_pack_entry& src, const xseg* sp) {
        const ghx_field_desc &f = en.field, &g = src.field;
        const std::string who = "contribution entry " + std::to_string(e) + " and its source ";
        validate_field(g);
        if (src.n_boxes < 0 || (src.n_boxes > 0 && !src.boxes)) throw invalid("bad boxes");
        if (en.n_boxes != src.n_boxes) throw invalid(who + "differ in their number of boxes");
        if (f.elem_size != g.elem_size) throw invalid(who + "differ in elem_size");
        if (f.dim != g.dim || f.num_components != g.num_components || (f.has_components != 0) != (g.has_components != 0))
            throw invalid(who + "differ in their dimensions or components");
        for (int d = 0; d < f.dim; ++d)
            if (f.layout[d] != g.layout[d]) throw invalid(who + "differ in layout order");
        const int spatial = f.dim - (f.has_components ? 1 : 0);
        for (int b = 0; !sp && b < en.n_boxes; ++b)
            for (int d = 0; d < spatial; ++d)
                if (int64_t(en.boxes[b].last[d]) - en.boxes[b].first[d] != int64_t(src.boxes[b].last[d]) - src.boxes[b].first[d])
                    throw invalid(who + "differ in the extents of box " + std::to_string(b));
        add_entry(src, e, k_src);
        // the entry's boxes are the last n_boxes of its slot's sums, the source's of its slot's sources
        std::vector<cbox>& sum = slots[en.field_slot].sum;
        const std::vector<cbox>& from = slots[src.field_slot].src;
        for (int b = 0; b < en.n_boxes; ++b)
        {
            cbox& c = sum[sum.size() - size_t(en.n_boxes) + size_t(b)];
            const cbox& q = from[from.size() - size_t(en.n_boxes) + size_t(b)];
            c.field_src = true;
            c.buf_slot = q.buf_slot;
            c.buf_off = q.buf_off;
            for (int d = 0; d < f.dim; ++d) c.bstride[d] = q.bstride[d];
            if (!sp) continue;
            // a cubed-sphere space: axis a of its dense box is the sender's dim by_speed[a]. The map
            // cell -> halo cell must be a bijection of the box onto the source box q: every axis
            // runs along one dim of q of the same extent, and the first cell's image is q's corner
            // at the first or, along a reversed axis, the last coordinate
            const xseg& x = sp[b];
            const int D = f.dim;
            int by_speed[GHX_MAX_DIM];
            for (int d = 0; d < D; ++d) by_speed[D - 1 - f.layout[d]] = d;
            const std::string shape = who + "differ in shape under the tile transform (box " + std::to_string(b) + ")";
            bool used[GHX_MAX_DIM] = {};
            int64_t origin = 0;
            bool moved = x.neg_mask != 0;
            for (int a = 0; a < D; ++a)
            {
                const int d = by_speed[a];
                const int64_t ext = c.last[d] - c.first[d] + 1;
                if (int64_t(x.ext[a]) != ext) throw invalid(shape);
                int to = -1;
                for (int r = 0; r < D && to < 0; ++r)
                    if (!used[r] && q.last[r] - q.first[r] + 1 == ext &&
                        (x.stride[a] == g.byte_strides[r] || x.stride[a] == -g.byte_strides[r]))
                        to = r;
                if (to < 0) throw invalid(shape);
                used[to] = true;
                const bool up = x.stride[a] == g.byte_strides[to];
                origin += ((up ? q.first[to] : q.last[to]) + (to < spatial ? g.offsets[to] : 0)) * g.byte_strides[to];
                c.bstride[d] = uint64_t(x.stride[a]);
                moved = moved || to != d || !up;
            }
            if (origin != x.field_off)
                throw invalid(who + "differ in shape under the tile transform (the image of box " + std::to_string(b) +
                              " is not its source box)");
            c.buf_off = uint64_t(x.field_off);
            c.neg = x.neg_mask;
            if (moved) ++n_rotated_sources;
        }
    };
    for (int e = 0; e < n; ++e)
    {
        const ghx_pack_entry& en = contrib[e];
        const int sz = dtype_size(dtypes[e]);
        if (!sz) throw invalid("unknown dtype code " + std::to_string(dtypes[e]) + " (GHX_DT_F32, _F64, _I32, _I64)");
        if (sz != en.field.elem_size)
            throw invalid("dtype code " + std::to_string(dtypes[e]) + " has " + std::to_string(sz) +
                          " bytes, the entry's elem_size is " + std::to_string(en.field.elem_size));
        const ghx_pack_entry* src = source ? source[e] : nullptr;
        add_entry(en, uint32_t(e), k_sum, src != nullptr);
        int32_t& dt = slots[en.field_slot].dtype;
        if (dt && dt != dtypes[e])
            throw invalid("two entries of field slot " + std::to_string(en.field_slot) + " differ in their dtype");
        dt = dtypes[e];
        if (src)
        {
            pair_entry(en, uint32_t(e), *src, space ? space[e] : nullptr);
            ++n_field_sources;
            continue;
        }
        if (en.buffer_offset % uint64_t(sz)) throw invalid("buffer offset is not a multiple of the element size");
        max_buf_slot = std::max(max_buf_slot, en.buffer_slot);
        buf_elem[en.buffer_slot] = std::max(buf_elem[en.buffer_slot], uint8_t(sz));
    }
    for (int k = 0; k < n_zero; ++k)
    {
        if (zero[k].field.elem_size != 4 && zero[k].field.elem_size != 8)
            throw invalid("a zero entry's elem_size is " + std::to_string(zero[k].field.elem_size) +
                          ", not that of a dtype (4 or 8)");
        add_entry(zero[k], uint32_t(k), k_zero);
        bool is_src = false;
        for (int e = 0; source && !is_src && e < n; ++e) is_src = source[e] && same_boxes(*source[e], zero[k]);
        slot_boxes& sb = slots[zero[k].field_slot];
        sb.zero_is_src.resize(sb.zero.size(), is_src ? 1 : 0);
    }
    // no cell is both summed and zeroed: box against box
    for (const auto& kv : slots)
    {
        const int spatial = kv.second.desc->dim - (kv.second.desc->has_components ? 1 : 0);
        for (const cbox& a : kv.second.sum)
            for (const cbox& z : kv.second.zero)
            {
                if (meet(a, z, spatial))
                    throw invalid("a cell of field slot " + std::to_string(kv.first) + " is both summed and zeroed (box " +
                                  std::to_string(a.box) + " of contribution entry " + std::to_string(a.entry) +
                                  " meets box " + std::to_string(z.box) + " of zero entry " + std::to_string(z.entry) + ")");
            }
    }
    // a get plan reads and zeroes a source cell in place: race-free only when exactly one (cell,
    // source) pair reads it and nothing else of the launch touches it
    for (const auto& kv : slots)
    {
        const slot_boxes& sb = kv.second;
        const int spatial = sb.desc->dim - (sb.desc->has_components ? 1 : 0);
        const std::string slot = "field slot " + std::to_string(kv.first);
        auto name = [](const cbox& c) { return "box " + std::to_string(c.box) + " of the source of contribution entry " + std::to_string(c.entry); };
        for (size_t i = 0; i < sb.src.size(); ++i)
        {
            const cbox& a = sb.src[i];
            for (size_t j = i + 1; j < sb.src.size(); ++j)
                if (meet(a, sb.src[j], spatial))
                    throw invalid("two source boxes of " + slot + " meet (" + name(a) + ", " + name(sb.src[j]) + ")");
            for (const cbox& c : sb.sum)
                if (meet(a, c, spatial))
                    throw invalid("a source box of " + slot + " meets a contribution box (" + name(a) + ", box " +
                                  std::to_string(c.box) + " of contribution entry " + std::to_string(c.entry) + ")");
            for (size_t z = 0; z < sb.zero.size(); ++z)
                if (!sb.zero_is_src[z] && meet(a, sb.zero[z], spatial))
                    throw invalid("a source box of " + slot + " meets a zero box (" + name(a) + ", box " +
                                  std::to_string(sb.zero[z].box) + " of zero entry " + std::to_string(sb.zero[z].entry) + ")");
        }
    }
    // the source pointer table of a get plan: the buffer slots that are read, then the source
    // field slots; a plan without sources indexes the buffers themselves
    int32_t tab_of_buf[GHX_MAX_SLOTS], tab_of_field[GHX_MAX_SLOTS];
    for (int b = 0; b < GHX_MAX_SLOTS; ++b) tab_of_buf[b] = get ? -1 : b, tab_of_field[b] = -1;
    if (get)
    {
        for (int b = 0; b < GHX_MAX_SLOTS; ++b)
            if (buf_elem[b])
            {
                tab_of_buf[b] = int32_t(tab_slot.size());
                tab_slot.push_back(b);
            }
        tab_field = uint32_t(tab_slot.size());
        for (const auto& kv : slots)
            if (!kv.second.src.empty())
            {
                tab_of_field[kv.first] = int32_t(tab_slot.size());
                tab_slot.push_back(kv.first);
            }
        if (tab_slot.size() > size_t(GHX_MAX_SLOTS))
            throw invalid("a get plan takes at most 64 source slots (the buffers it reads and its source fields, one launch)");
    }

    const uint32_t tb = std::max<uint32_t>(1, g_tune.tile_bytes);
    // one sub-box (spatial bounds first / last, sources `list` into `from`) -> box, source and
    // tile records
    auto emit = [&](int32_t slot, const slot_boxes& sb, const int64_t* first, const int64_t* last,
                    const std::vector<cbox>& from, const std::vector<uint32_t>& list, bool is_zero) {
        const ghx_field_desc& f = *sb.desc;
        const int D = f.dim, spatial = D - (f.has_components ? 1 : 0);
        const int64_t elem = f.elem_size;
        int by_speed[GHX_MAX_DIM];
        for (int d = 0; d < D; ++d) by_speed[D - 1 - f.layout[d]] = d;
        int64_t ext[GHX_MAX_DIM], lo[GHX_MAX_DIM];
        for (int d = 0; d < D; ++d)
        {
            lo[d] = d < spatial ? first[d] : 0;
            ext[d] = d < spatial ? last[d] - first[d] + 1 : f.num_components;
        }
        if (uint64_t(srcs.size()) + list.size() > kMaxRecords) throw invalid("more than 2^32 - 1 source records");
        const uint32_t first_src = uint32_t(srcs.size());
        // rows along the layout's fastest dim; a strided fastest dim makes every element a row
        const int cont = by_speed[0];
        bool unit = f.byte_strides[cont] == elem;
        for (uint32_t j : list) unit = unit && from[j].bstride[cont] == uint64_t(elem);  // a strided source field
        // a source that negates some components of a vector and not the others: the component
        // dimension stays a tile axis of its own, and where it is the row the lanes take elements
        const int comp = f.has_components ? D - 1 : -1;
        bool mixed = false;
        for (uint32_t j : list) mixed = mixed || (from[j].neg && f.num_components > 1);
        const bool comp_row = mixed && unit && cont == comp;
        int64_t L = unit ? ext[cont] * elem : elem;
        int outer[GHX_MAX_DIM];
        int n_outer = 0;
        for (int k = unit ? 1 : 0; k < D; ++k)
            if (ext[by_speed[k]] > 1) outer[n_outer++] = by_speed[k];
        // rows that are adjacent in the field and in every source's buffer box are one row
        auto mergeable = [&] {
            if (n_outer == 0 || f.byte_strides[outer[0]] != L || L * ext[outer[0]] >= (int64_t(1) << 30)) return false;
            if (mixed && (comp_row || outer[0] == comp)) return false;
            for (uint32_t j : list)
                if (from[j].bstride[outer[0]] != uint64_t(L)) return false;
            return true;
        };
        while (mergeable())
        {
            L *= ext[outer[0]];
            for (int k = 1; k < n_outer; ++k) outer[k - 1] = outer[k];
            --n_outer;
        }
        if (L >= (int64_t(1) << 31)) throw invalid("row too long");
        sacc_tile t{};
        uint64_t rows = 1;
        int w = wlog2_of(uint64_t(L));
        if (comp_row) w = std::min(w, wlog2_of(uint64_t(elem)));
        t.comp = comp_row ? kSaccCompRow : kSaccCompNone;
        for (int k = 0; mixed && !comp_row && k < n_outer; ++k)
            if (outer[k] == comp) t.comp = uint8_t(1 + k);
        for (int d = 0; d < D; ++d) t.field_off += (lo[d] + (d < spatial ? f.offsets[d] : 0)) * f.byte_strides[d];
        w = std::min(w, wlog2_of(uint64_t(t.field_off)));
        for (int k = 0; k < 4; ++k)
        {
            t.stride[k] = k < n_outer ? f.byte_strides[outer[k]] : 0;
            t.ext[k] = k < n_outer ? uint32_t(ext[outer[k]]) : 1;
            rows *= t.ext[k];
            if (k < n_outer) w = std::min(w, wlog2_of(uint64_t(t.stride[k])));
        }
        if (rows > kMaxRecords) throw invalid("a sub-box has more than 2^32 - 1 rows");
        for (uint32_t j : list)
        {
            const cbox& c = from[j];
            sacc_src s{};
            s.buf_off = c.buf_off;
            for (int d = 0; d < spatial; ++d) s.buf_off += uint64_t(lo[d] - c.first[d]) * c.bstride[d];
            s.buf_slot = uint32_t(c.field_src ? tab_of_field[c.buf_slot] : tab_of_buf[c.buf_slot]);
            s.flags = (c.field_src ? kSaccFieldSrc : 0) | (uint32_t(c.neg) << kSaccNegShift);
            w = std::min(w, wlog2_of(s.buf_off));
            for (int k = 0; k < n_outer; ++k)
            {
                s.stride[k] = c.bstride[outer[k]];
                w = std::min(w, wlog2_of(s.stride[k]));
            }
            t.buf_mask |= uint64_t(1) << s.buf_slot;
            srcs.push_back(s);
            source_map m{};
            for (int d = 0; d < D; ++d) m.stride[d] = int64_t(c.bstride[d]);
            m.neg = c.neg;
            m.comp_dim = int8_t(comp);
            src_map.push_back(m);
            src_entry.push_back(c.entry);
            src_box.push_back(c.box);
        }
        for (int k = 0; k < 3; ++k) t.mag_ext[k] = make_magic(t.ext[k]);
        t.first_src = first_src;
        t.n_src = uint32_t(list.size());
        t.field_slot = uint16_t(slot);
        t.zero = is_zero ? 1 : 0;
        t.dtype = uint8_t(is_zero ? (elem == 8 ? GHX_DT_I64 : GHX_DT_I32) : sb.dtype);
        t.wlog2 = uint8_t(w);
        t.n_outer = uint8_t(n_outer);
        saccum_box bx{};
        bx.field_slot = slot;
        bx.zero = is_zero;
        for (int d = 0; d < spatial; ++d)
        {
            bx.first[d] = int32_t(first[d]);
            bx.last[d] = int32_t(last[d]);
        }
        bx.row_elems = uint64_t(L / elem);
        bx.wlog2 = uint8_t(w);
        bx.first_src = first_src;
        bx.n_src = t.n_src;
        boxes.push_back(bx);
        max_sources = std::max(max_sources, t.n_src);
        bytes += rows * uint64_t(L) * list.size();
        // tiles: whole rows of tile_bytes field bytes; a row longer than that in pieces
        auto push = [&](uint32_t row, uint32_t nr, uint32_t col0, uint32_t len) {
            if (tiles.size() >= kMaxRecords) throw invalid("more than 2^32 - 1 tiles");
            t.first_row = row;
            t.n_rows = nr;
            t.col0 = col0;
            t.len = len;
            t.mag_vec = make_magic(len >> w);
            tiles.push_back(t);
        };
        if (uint64_t(L) > tb)
        {
            const uint32_t piece = std::max<uint32_t>(16, tb - tb % 16);
            for (uint64_t r = 0; r < rows; ++r)
                for (uint32_t c0 = 0; c0 < uint32_t(L); c0 += piece)
                    push(uint32_t(r), 1, c0, std::min(piece, uint32_t(L) - c0));
        }
        else
        {
            const uint64_t per = std::max<uint64_t>(1, tb / uint64_t(L));
            for (uint64_t r = 0; r < rows; r += per) push(uint32_t(r), uint32_t(std::min(per, rows - r)), 0, uint32_t(L));
        }
    };

    // the arrangement, per field slot: every dimension cut at every box's first and last + 1; an
    // elementary box lies in a contribution box or outside it. Boxes come in ascending (entry,
    // box), so every list ascends. Elementary boxes adjacent along the fastest spatial dimension
    // with equal lists are merged.
    for (const auto& kv : slots)
    {
        const slot_boxes& sb = kv.second;
        if (sb.sum.empty()) continue;
        const ghx_field_desc& f = *sb.desc;
        const int spatial = f.dim - (f.has_components ? 1 : 0);
        int order[GHX_MAX_DIM];  // spatial dims, slowest first
        int no = 0;
        for (int l = 0; l < f.dim; ++l)
            for (int d = 0; d < spatial; ++d)
                if (f.layout[d] == l) order[no++] = d;
        std::vector<int64_t> cuts[GHX_MAX_DIM];
        for (int d = 0; d < spatial; ++d)
        {
            for (const cbox& c : sb.sum)
            {
                cuts[d].push_back(c.first[d]);
                cuts[d].push_back(c.last[d] + 1);
            }
            std::sort(cuts[d].begin(), cuts[d].end());
            cuts[d].erase(std::unique(cuts[d].begin(), cuts[d].end()), cuts[d].end());
        }
        using key = std::array<uint32_t, GHX_MAX_DIM>;  // interval index per dim of `order`
        std::map<key, std::vector<uint32_t>> cells;
        for (uint32_t j = 0; j < sb.sum.size(); ++j)
        {
            const cbox& c = sb.sum[j];
            uint32_t lo[GHX_MAX_DIM] = {}, hi[GHX_MAX_DIM] = {1, 1, 1, 1};
            for (int k = 0; k < spatial; ++k)
            {
                const std::vector<int64_t>& cu = cuts[order[k]];
                lo[k] = uint32_t(std::lower_bound(cu.begin(), cu.end(), c.first[order[k]]) - cu.begin());
                hi[k] = uint32_t(std::lower_bound(cu.begin(), cu.end(), c.last[order[k]] + 1) - cu.begin());
            }
            key i{};
            for (i[0] = lo[0]; i[0] < hi[0]; ++i[0])
                for (i[1] = lo[1]; i[1] < hi[1]; ++i[1])
                    for (i[2] = lo[2]; i[2] < hi[2]; ++i[2])
                        for (i[3] = lo[3]; i[3] < hi[3]; ++i[3]) cells[i].push_back(j);
        }
        const int fast = spatial - 1;  // position in `order` of the fastest spatial dim
        auto it = cells.begin();
        while (it != cells.end())
        {
            key a = it->first;
            uint32_t end = a[fast] + 1;
            auto nx = std::next(it);
            for (; nx != cells.end(); ++nx, ++end)
            {
                key b = nx->first;
                const bool follows = b[fast] == end;
                b[fast] = a[fast];
                if (!follows || b != a || nx->second != it->second) break;
            }
            int64_t first[GHX_MAX_DIM] = {}, last[GHX_MAX_DIM] = {};
            for (int k = 0; k < spatial; ++k)
            {
                first[order[k]] = cuts[order[k]][a[k]];
                last[order[k]] = cuts[order[k]][(k == fast ? end : a[k] + 1)] - 1;
            }
            emit(kv.first, sb, first, last, sb.sum, it->second, false);
            it = nx;
        }
    }
    n_sum_boxes = uint32_t(boxes.size());
    n_sum_tiles = uint32_t(tiles.size());
    for (const auto& kv : slots)
        for (size_t z = 0; z < kv.second.zero.size(); ++z)
            if (!kv.second.zero_is_src[z])
                emit(kv.first, kv.second, kv.second.zero[z].first, kv.second.zero[z].last, kv.second.zero, {}, true);

    if (tiles.empty() || !have_device()) return;
    to_device(dev.tiles, tiles, "accumulate tiles");
    to_device(dev.srcs, srcs, "accumulate sources");
}

int saccum_plan::execute(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const
{
    if (get) throw invalid("a get plan (ghx_saccum_get_create) runs through ghx_saccum_get_execute");
    return launch(fptr, nf, bptr, nb, zero_halos, stream);
}

int saccum_plan::execute_get(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const
{
    if (!get) throw invalid("not a get plan (ghx_saccum_get_create)");
    return launch(fptr, nf, bptr, nb, zero_halos, stream);
}

// k_accum_s, or of a get plan k_accum_get_s (k_accum_get_x: a plan with cubed-sphere spaces)
int saccum_plan::launch(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const
{
    const uint32_t n_tiles = zero_halos ? uint32_t(tiles.size()) : n_sum_tiles;
    if (n_tiles == 0) return GHX_OK;
    if (!fptr || (!bptr && max_buf_slot >= 0) || nf <= max_field_slot || nb <= max_buf_slot)
        throw invalid("pointer arrays do not cover the plan's slots");
    kargs_sa a{};
    a.n_tiles = n_tiles;
    a.zero_src = get && zero_halos ? 1 : 0;
    for (int s = 0; s <= max_field_slot; ++s)
    {
        if (!slot_elem[s]) continue;
        if (!fptr[s]) throw invalid("null field pointer");
        a.field_ptr[s] = reinterpret_cast<uint64_t>(fptr[s]);
        if (a.field_ptr[s] % slot_elem[s]) throw invalid("a field pointer is not aligned to its element");
    }
    // the source pointer table: the buffers at their own slots, or a get plan's tab_slot (the
    // buffers that are read, then the source fields)
    const uint32_t n_tab = get ? uint32_t(tab_slot.size()) : uint32_t(max_buf_slot + 1);
    for (uint32_t t = 0; t < n_tab; ++t)
    {
        const int32_t s = get ? tab_slot[t] : int32_t(t);
        if (get && t >= tab_field) a.buf_ptr[t] = a.field_ptr[s];  // checked above
        else
        {
            if (!buf_elem[s]) continue;  // a buffer no entry reads (tab_slot names none)
            if (!bptr[s]) throw invalid("null buffer pointer");
            a.buf_ptr[t] = reinterpret_cast<uint64_t>(bptr[s]);
            if (a.buf_ptr[t] % buf_elem[s]) throw invalid("a buffer pointer is not aligned to its elements");
        }
        if (a.buf_ptr[t] % 8) a.buf_mis8 |= uint64_t(1) << t;
        if (a.buf_ptr[t] % 16) a.buf_mis16 |= uint64_t(1) << t;
    }
    if (!dev.tiles) throw hip_error("plan has no device tables (no HIP device at creation)");
    a.tiles = static_cast<const sacc_tile*>(dev.tiles);
    a.srcs = static_cast<const sacc_src*>(dev.srcs);
    const uint32_t grid = grid_for_tiles(n_tiles);
    if (!get) return launch_accum_s(a, stream, grid);
    return rotated ? launch_accum_get_x(a, stream, grid) : launch_accum_get_s(a, stream, grid);
}

}  // namespace ghx
