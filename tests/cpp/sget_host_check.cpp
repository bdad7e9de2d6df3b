// sget_host_check — stand-alone host program (its own main; links the library's sources) for the
// get-accumulate plan: ghx_saccum_get_create / _info / _source_kind / _destroy, created without a
// device. The plans of one periodic N^D domain whose every message is a self message, and of a
// plan that mixes field sources with a buffer, are replayed on host arrays from their TILE and
// SOURCE records — the records a launch reads, through the kernel's own decode (ghx_addr.hpp) at
// the planned vector width and at every narrower one, every access bounds-checked — and compared
// with the definition (every message gathered from the halo cells first). The replay counts: every
// source cell is read once and lies inside a receive box, every owner cell is written once. Built
// with -fsanitize=address,undefined by tools/cs_host_sanitize.sh; needs no GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ghex_amd/csrc/ghx_addr.hpp"
#include "../../ghex_amd/csrc/ghx_plan.hpp"

#define CHECK(c)                                                                  \
    do                                                                            \
    {                                                                             \
        if (!(c))                                                                 \
        {                                                                         \
            std::printf("%s:%d: CHECK failed: %s (%s)\n", __FILE__, __LINE__, #c, \
                        ghx_last_error());                                        \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

namespace
{
struct field
{
    ghx_field_desc d{};
    int64_t n_elems = 0;
};

field make_field(int D, int E, int H, int elem, const int* layout, int ncomp, int fast)
{
    field f;
    const int nd = D + (ncomp ? 1 : 0);
    f.d.dim = nd;
    f.d.elem_size = elem;
    f.d.num_components = ncomp ? ncomp : 1;
    f.d.has_components = ncomp ? 1 : 0;
    int64_t s = fast;
    for (int v = nd - 1; v >= 0; --v)
        for (int d = 0; d < nd; ++d)
            if (layout[d] == v)
            {
                const int ext = d < D ? E : ncomp;
                f.d.layout[d] = v;
                f.d.byte_strides[d] = s * elem;
                f.d.offsets[d] = d < D ? H : 0;
                f.d.extents[d] = ext;
                s *= ext;
            }
    f.n_elems = s;
    return f;
}

// the 26 (8 in 2-D) send boxes and receive boxes of one periodic N^D domain with halo H, paired
void periodic_boxes(int D, int N, int H, std::vector<ghx_box>& send, std::vector<ghx_box>& recv)
{
    int dir[3];
    const int lo = D > 2 ? -1 : 0, hi = D > 2 ? 1 : 0;
    for (dir[2] = lo; dir[2] <= hi; ++dir[2])
        for (dir[1] = -1; dir[1] <= 1; ++dir[1])
            for (dir[0] = -1; dir[0] <= 1; ++dir[0])
            {
                if (!dir[0] && !dir[1] && !dir[2]) continue;
                ghx_box s{}, r{};
                for (int d = 0; d < D; ++d)
                {
                    r.first[d] = dir[d] < 0 ? -H : dir[d] > 0 ? N : 0;
                    r.last[d] = dir[d] < 0 ? -1 : dir[d] > 0 ? N + H - 1 : N - 1;
                    s.first[d] = dir[d] < 0 ? N - H : 0;
                    s.last[d] = dir[d] > 0 ? H - 1 : N - 1;
                }
                send.push_back(s);
                recv.push_back(r);
            }
}

// element indices in the field of the box's cells, in the order of its dense buffer box
void box_cells(const ghx_field_desc& f, const ghx_box& b, std::vector<int64_t>& out)
{
    const int D = f.dim, sp = D - (f.has_components ? 1 : 0);
    int order[GHX_MAX_DIM];  // slowest first
    for (int d = 0; d < D; ++d) order[f.layout[d]] = d;
    int64_t first[GHX_MAX_DIM], ext[GHX_MAX_DIM], c[GHX_MAX_DIM] = {};
    int64_t n = 1;
    for (int d = 0; d < D; ++d)
    {
        first[d] = d < sp ? b.first[d] + f.offsets[d] : 0;
        ext[d] = d < sp ? b.last[d] - b.first[d] + 1 : f.num_components;
        n *= ext[d];
    }
    for (int64_t i = 0; i < n; ++i)
    {
        int64_t e = 0;
        for (int d = 0; d < D; ++d) e += (first[d] + c[d]) * (f.byte_strides[d] / f.elem_size);
        out.push_back(e);
        for (int k = D - 1; k >= 0; --k)
        {
            const int d = order[k];
            if (++c[d] < ext[d]) break;
            c[d] = 0;
        }
    }
}

template<typename T>
T value(uint64_t i)
{
    const uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull;
    return T(int64_t(h >> 40) % 2001 - 1000);  // integer-valued: every sum is exact and order-free
}

// the definition: every message gathered from its source (the halo cells before the launch, or the
// buffer), then for (entry, box) ascending field[cell] += message cell; then zeros
template<typename T>
void definition(std::vector<std::vector<T>>& F, const std::vector<T>& buf, const std::vector<ghx_pack_entry>& contrib,
                const std::vector<const ghx_pack_entry*>& source, const std::vector<ghx_pack_entry>& zero, bool zero_halos)
{
    std::vector<std::vector<T>> msg(contrib.size());
    for (size_t e = 0; e < contrib.size(); ++e)
    {
        const ghx_pack_entry& en = contrib[e];
        size_t at = size_t(en.buffer_offset / sizeof(T));
        for (int b = 0; b < en.n_boxes; ++b)
        {
            std::vector<int64_t> cells;
            if (source[e])
            {
                box_cells(source[e]->field, source[e]->boxes[b], cells);
                for (int64_t c : cells) msg[e].push_back(F.at(size_t(source[e]->field_slot)).at(size_t(c)));
            }
            else
            {
                box_cells(en.field, en.boxes[b], cells);
                for (size_t i = 0; i < cells.size(); ++i) msg[e].push_back(buf.at(at++));
            }
        }
    }
    for (size_t e = 0; e < contrib.size(); ++e)
    {
        size_t at = 0;
        for (int b = 0; b < contrib[e].n_boxes; ++b)
        {
            std::vector<int64_t> cells;
            box_cells(contrib[e].field, contrib[e].boxes[b], cells);
            for (int64_t c : cells)
            {
                T& v = F.at(size_t(contrib[e].field_slot)).at(size_t(c));
                v = T(v + msg[e].at(at++));
            }
        }
    }
    if (!zero_halos) return;
    for (const ghx_pack_entry& z : zero)
        for (int b = 0; b < z.n_boxes; ++b)
        {
            std::vector<int64_t> cells;
            box_cells(z.field, z.boxes[b], cells);
            for (int64_t c : cells) F.at(size_t(z.field_slot)).at(size_t(c)) = T(0);
        }
}

// the launch on the host: every tile record at vector width 1 << w, every access checked against
// its array. reads[slot][cell]: how often a field source read the cell; writes: owner stores
template<typename T>
void replay(const ghx::saccum_plan& p, std::vector<std::vector<T>>& F, const std::vector<T>& buf, bool zero_halos,
            int narrow_by, std::vector<std::vector<int>>& reads, std::vector<std::vector<int>>& writes)
{
    CHECK(p.get);
    const size_t n_tiles = zero_halos ? p.tiles.size() : p.n_sum_tiles;
    int elog2 = 0;
    while ((1u << elog2) < sizeof(T)) ++elog2;
    for (size_t t = 0; t < n_tiles; ++t)
    {
        const ghx::sacc_tile& s = p.tiles[t];
        CHECK(s.wlog2 >= elog2 && s.wlog2 <= 4 && s.len % (1u << s.wlog2) == 0 && s.len > 0 && s.n_rows > 0);
        const int w = std::max(elog2, int(s.wlog2) - narrow_by);
        CHECK((t < p.n_sum_tiles) == (s.zero == 0) && (s.zero == 0) == (s.n_src > 0));
        std::vector<T>& cellv = F.at(s.field_slot);
        const uint32_t nv = ghx::sacc_vectors(s, w);
        CHECK(uint64_t(nv) << w == uint64_t(s.n_rows) * s.len);
        for (uint32_t i = 0; i < nv; ++i)
        {
            uint32_t c[4], col;
            ghx::sacc_decode(s, i, w, c, col);
            CHECK(c[0] < s.ext[0] && c[1] < s.ext[1] && c[2] < s.ext[2] && c[3] < s.ext[3]);
            CHECK(col >= s.col0 && col + (1u << w) <= s.col0 + s.len);
            const int64_t foff = ghx::affine_offset(s.field_off, s.stride, c) + int64_t(col);
            CHECK(foff >= 0 && foff % int64_t(1u << w) == 0);
            for (uint32_t k = 0; k < (1u << w) / sizeof(T); ++k)
            {
                const size_t at = size_t(foff) / sizeof(T) + k;
                T& cell = cellv.at(at);
                ++writes.at(s.field_slot).at(at);
                if (s.zero)
                {
                    cell = T(0);
                    continue;
                }
                T acc = cell;
                for (uint32_t j = s.first_src; j < s.first_src + s.n_src; ++j)
                {
                    const ghx::sacc_src& r = p.srcs.at(j);
                    CHECK(r.buf_slot < p.tab_slot.size() && ((s.buf_mask >> r.buf_slot) & 1u));
                    const bool from_field = (r.flags & ghx::kSaccFieldSrc) != 0;
                    CHECK(from_field == (r.buf_slot >= p.tab_field) && (r.flags & ~ghx::kSaccFieldSrc) == 0);
                    const uint64_t off = r.buf_off + uint64_t(c[0]) * r.stride[0] + uint64_t(c[1]) * r.stride[1] +
                                         uint64_t(c[2]) * r.stride[2] + uint64_t(c[3]) * r.stride[3] + col;
                    CHECK(off % (1u << w) == 0);
                    const size_t from = size_t(off) / sizeof(T) + k;
                    if (!from_field)
                    {
                        acc = T(acc + buf.at(from));
                        continue;
                    }
                    const size_t slot = size_t(p.tab_slot[r.buf_slot]);
                    T& halo = F.at(slot).at(from);
                    CHECK(++reads.at(slot).at(from) == 1);  // read once: its value is the launch's input
                    acc = T(acc + halo);
                    if (zero_halos) halo = T(0);
                }
                cell = acc;
            }
        }
    }
}

template<typename T>
void run(const std::vector<field>& fields, const std::vector<ghx_pack_entry>& contrib,
         const std::vector<const ghx_pack_entry*>& source, const std::vector<ghx_pack_entry>& zero, int32_t code,
         size_t buf_elems, int64_t n_zero_boxes)
{
    std::vector<int32_t> dt(contrib.size(), code);
    ghx_saccum* p = nullptr;
    CHECK(ghx_saccum_get_create(contrib.data(), dt.data(), source.data(), int32_t(contrib.size()), zero.data(),
                                int32_t(zero.size()), &p) == GHX_OK && p);
    int64_t nb = 0, nz = 0, ns = 0;
    CHECK(ghx_saccum_info(p, nullptr, &nb, &nz, &ns, nullptr, nullptr) == GHX_OK && nz == n_zero_boxes && nb > 0);
    for (int64_t j = 0; j < ns; ++j)
    {
        int32_t e = -1, kind = -1, slot = -1;
        uint64_t off = 0, off2 = 1;
        CHECK(ghx_saccum_source(p, j, &e, nullptr, nullptr, &off) == GHX_OK);
        CHECK(ghx_saccum_source_kind(p, j, &kind, &slot, &off2) == GHX_OK && off == off2);
        CHECK(kind == (source[size_t(e)] ? 1 : 0));
        CHECK(slot == (source[size_t(e)] ? source[size_t(e)]->field_slot : contrib[size_t(e)].buffer_slot));
    }
    CHECK(ghx_saccum_source_kind(p, ns, nullptr, nullptr, nullptr) == GHX_ERR_INVALID);
    CHECK(ghx_saccum_source_kind(p, -1, nullptr, nullptr, nullptr) == GHX_ERR_INVALID);
    // which cells receive boxes of sources hold, and which cells contribution boxes hold
    std::vector<std::vector<int>> in_recv, in_send;
    for (const field& f : fields)
    {
        in_recv.emplace_back(size_t(f.n_elems), 0);
        in_send.emplace_back(size_t(f.n_elems), 0);
    }
    for (size_t e = 0; e < contrib.size(); ++e)
        for (int b = 0; b < contrib[e].n_boxes; ++b)
        {
            std::vector<int64_t> cells;
            box_cells(contrib[e].field, contrib[e].boxes[b], cells);
            for (int64_t c : cells) in_send[size_t(contrib[e].field_slot)][size_t(c)] = 1;
            if (!source[e]) continue;
            cells.clear();
            box_cells(source[e]->field, source[e]->boxes[b], cells);
            for (int64_t c : cells) ++in_recv[size_t(source[e]->field_slot)][size_t(c)];
        }
    for (int zero_halos = 0; zero_halos < 2; ++zero_halos)
        for (int narrow = 0; narrow < 3; ++narrow)
        {
            std::vector<std::vector<T>> want, got;
            for (size_t k = 0; k < fields.size(); ++k)
            {
                want.emplace_back(size_t(fields[k].n_elems));
                for (size_t i = 0; i < want[k].size(); ++i) want[k][i] = value<T>(i * 64 + k);
            }
            got = want;
            const std::vector<std::vector<T>> before = want;
            std::vector<T> buf(buf_elems);
            for (size_t i = 0; i < buf.size(); ++i) buf[i] = value<T>((i << 8) + 5);
            std::vector<std::vector<int>> reads, writes;
            for (const field& f : fields)
            {
                reads.emplace_back(size_t(f.n_elems), 0);
                writes.emplace_back(size_t(f.n_elems), 0);
            }
            definition(want, buf, contrib, source, zero, zero_halos != 0);
            replay(*p, got, buf, zero_halos != 0, narrow, reads, writes);
            for (size_t k = 0; k < fields.size(); ++k)
            {
                CHECK(want[k] == got[k]);
                CHECK(reads[k] == in_recv[k]);  // every source cell once, nothing outside a receive box
                for (size_t i = 0; i < writes[k].size(); ++i)
                    if (in_send[k][i]) CHECK(writes[k][i] == 1);  // every owner cell written once
                    else CHECK(writes[k][i] == 0 || (zero_halos && writes[k][i] == 1 && !in_recv[k][i]));
            }
            CHECK(before[0] != got[0]);
        }
    // without a device the plan cannot run; wrong pointer arrays and the other execute are refused
    CHECK(ghx_saccum_get_execute(p, nullptr, 0, nullptr, 0, 1, nullptr) == GHX_ERR_INVALID);
    void* some[2] = {&p, &p};
    CHECK(ghx_saccum_execute(p, some, 2, some, 2, 1, nullptr) == GHX_ERR_INVALID);
    CHECK(std::strstr(ghx_last_error(), "ghx_saccum_get_execute"));
    CHECK(ghx_saccum_destroy(p) == GHX_OK);
}

template<typename T>
void one_domain(int D, int N, int H, const int* layout, int ncomp, int fast, int32_t code)
{
    const field f = make_field(D, N + 2 * H, H, int(sizeof(T)), layout, ncomp, fast);
    std::vector<ghx_box> send, recv;
    periodic_boxes(D, N, H, send, recv);
    ghx_pack_entry c{}, z{};
    c.field = z.field = f.d;
    c.boxes = send.data();
    c.n_boxes = int32_t(send.size());
    c.buffer_slot = -3;  // a sourced entry: ignored
    z.boxes = recv.data();
    z.n_boxes = int32_t(recv.size());
    run<T>({f}, {c}, {&z}, {z}, code, 0, 0);
}

// the x faces of a 6^3 domain from another field's halos (other strides), its y faces from a buffer,
// a peer's zero entry beside them
template<typename T>
void mixed(int32_t code, int src_halo, int src_fast)
{
    const int xyz[3] = {2, 1, 0};
    const field f = make_field(3, 10, 2, int(sizeof(T)), xyz, 0, 1);
    const field g = make_field(3, 6 + 2 * src_halo, src_halo, int(sizeof(T)), xyz, 0, src_fast);
    auto box3 = [](int x0, int x1, int y0, int y1, int z0, int z1) {
        ghx_box b{};
        b.first[0] = x0, b.last[0] = x1, b.first[1] = y0, b.last[1] = y1, b.first[2] = z0, b.last[2] = z1;
        return b;
    };
    const ghx_box xs[2] = {box3(0, 1, 0, 5, 0, 5), box3(4, 5, 0, 5, 0, 5)};
    const ghx_box xr[2] = {box3(6, 7, 0, 5, 0, 5), box3(-2, -1, 0, 5, 0, 5)};
    const ghx_box ys[2] = {box3(0, 5, 0, 1, 0, 5), box3(0, 5, 4, 5, 0, 5)};
    const ghx_box yr[2] = {box3(0, 5, 6, 7, 0, 5), box3(0, 5, -2, -1, 0, 5)};
    ghx_pack_entry cx{}, cy{}, sx{}, zy{};
    cx.field = cy.field = zy.field = f.d;
    sx.field = g.d;
    sx.field_slot = 1;
    cx.boxes = xs, cy.boxes = ys, sx.boxes = xr, zy.boxes = yr;
    cx.n_boxes = cy.n_boxes = sx.n_boxes = zy.n_boxes = 2;
    cy.buffer_slot = 2;
    cy.buffer_offset = 2 * sizeof(T);
    run<T>({f, g}, {cx, cy}, {&sx, nullptr}, {sx, zy}, code, 2 + 2 * 6 * 2 * 6, 2);
}
}  // namespace

int main()
{
    const int xyz[3] = {2, 1, 0}, zyx[3] = {0, 1, 2}, yzx[3] = {1, 2, 0};
    const int comp_fast[4] = {2, 1, 0, 3}, comp_slow[4] = {3, 2, 1, 0}, xy[2] = {1, 0};
    one_domain<double>(3, 6, 2, xyz, 0, 1, GHX_DT_F64);
    one_domain<float>(3, 6, 1, xyz, 0, 1, GHX_DT_F32);
    one_domain<float>(3, 5, 3, xyz, 0, 1, GHX_DT_F32);
    one_domain<uint64_t>(3, 3, 2, xyz, 0, 1, GHX_DT_I64);
    one_domain<uint32_t>(3, 2, 2, zyx, 0, 1, GHX_DT_I32);
    one_domain<double>(3, 3, 2, yzx, 0, 1, GHX_DT_F64);
    one_domain<float>(3, 3, 2, comp_fast, 3, 1, GHX_DT_F32);
    one_domain<uint32_t>(3, 3, 2, comp_slow, 2, 1, GHX_DT_I32);
    one_domain<double>(3, 3, 2, xyz, 0, 2, GHX_DT_F64);  // strided fastest dim
    one_domain<float>(2, 7, 2, xy, 0, 1, GHX_DT_F32);
    ghx_tune("tile_bytes", 1024);  // several tiles per sub-box, a tile ending inside one
    one_domain<double>(3, 19, 2, xyz, 0, 1, GHX_DT_F64);
    one_domain<float>(2, 300, 2, xy, 0, 1, GHX_DT_F32);  // rows longer than a tile
    ghx_tune("reset", 0);
    mixed<double>(GHX_DT_F64, 2, 1);
    mixed<uint32_t>(GHX_DT_I32, 3, 1);
    mixed<uint64_t>(GHX_DT_I64, 2, 2);  // a strided source field: rows of one element
    std::printf("sget_host_check: OK\n");
    return 0;
}
