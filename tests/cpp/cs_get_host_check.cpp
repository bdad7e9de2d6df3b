// cs_get_host_check — stand-alone host program (its own main; links the library's sources) for the
// fused cubed-sphere adjoint (ghx_cs_exchange_adjoint_self_create, k_accum_get_x). It plans the
// cubed-sphere fixture geometries without a device, with all domains on one rank (form 1: every
// message a self message) and with tiles 0-2 on this rank and 3-5 on another (form 2: self and peer
// messages), and replays on the host EVERY TILE RECORD of the get plan with its source records — the
// records a launch reads, through the kernel's own decode (ghx_addr.hpp), at the planned vector
// width and at every narrower one, the sign taken from the record's mask and the lane's component
// index as the kernel takes it — every field and buffer access bounds-checked. It checks that
// every source cell is read once and is a cell of a receive box of a self message, that every
// owner cell (a cell of a send box) is written once and nothing else but the zeroed halo cells is
// written, that every address lies inside its field, and that the fields hold the definition,
// computed from the reference's geometry (cs_check.hpp): S[cell] += s_k * R[T^-1(cell)] for a
// self message, S[cell] += B[cell] for a peer's, then zeros. Values are small integers in every
// element type, so the sums are exact in any order. Built with -fsanitize=address,undefined by
// tools/cs_host_sanitize.sh; needs no GPU.
#include <algorithm>

#include "cs_check.hpp"

using namespace cs_check;

namespace
{
// the element at `p` as an integer, and back, in the field's type
int64_t load(const spec& s, const unsigned char* p)
{
    if (s.kind == 2 && s.elem == 4) { int32_t v; std::memcpy(&v, p, 4); return v; }
    if (s.kind == 2) { int64_t v; std::memcpy(&v, p, 8); return v; }
    if (s.elem == 4) { float v; std::memcpy(&v, p, 4); return int64_t(v); }
    double v;
    std::memcpy(&v, p, 8);
    return int64_t(v);
}
void store(const spec& s, unsigned char* p, int64_t x)
{
    if (s.kind == 2 && s.elem == 4) { const int32_t v = int32_t(x); std::memcpy(p, &v, 4); }
    else if (s.kind == 2) std::memcpy(p, &x, 8);
    else if (s.elem == 4) { const float v = float(x); std::memcpy(p, &v, 4); }
    else { const double v = double(x); std::memcpy(p, &v, 8); }
}
int64_t small(uint64_t i)
{
    const uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull;
    return int64_t(h >> 40) % 2001 - 1000;
}

void run(const config& cfg, const int* layout, const std::vector<spec>& specs, bool two_ranks, uint32_t tile_bytes)
{
    fixture fx(cfg, layout, specs);
    if (!fx.pat) return;
    if (two_ranks)
    {
        ghx_pattern_destroy(fx.pat);
        fx.pat = nullptr;
        for (ghx_cs_domain& d : fx.doms) d.rank = d.tile / 3;
        CHECK(ghx_cs_pattern_create(cfg.c, cfg.levels, fx.doms.data(), int(fx.doms.size()), cfg.halos, 0, &fx.pat) == GHX_OK);
        if (!fx.pat) return;
        std::vector<field> mine;
        for (field& f : fx.fields)
            if (fx.doms[size_t(f.dom)].rank == 0) mine.push_back(std::move(f));
        fx.fields = std::move(mine);
    }
    size_t n_mine = 0;
    for (const ghx_cs_domain& d : fx.doms) n_mine += d.rank == 0;
    for (size_t i = 0; i < fx.fields.size(); ++i)
    {
        field& f = fx.fields[i];
        for (size_t o = 0; o + size_t(f.sp.elem) <= f.mem.size(); o += size_t(f.sp.elem))
            store(f.sp, f.mem.data() + o, small(o * 64 + i));
        f.first = f.want = f.mem;
    }
    std::vector<ghx_exchange_item> items;
    std::vector<ghx_cs_item> cs;
    fx.items(items, cs);
    ghx_exchange* ex = nullptr;
    CHECK(ghx_cs_exchange_create(items.data(), cs.data(), int(items.size()), &ex) == GHX_OK);
    if (!ex) return;
    std::vector<int32_t> dtypes;
    for (const field& f : fx.fields)
        dtypes.push_back(f.sp.kind == 2 ? (f.sp.elem == 4 ? GHX_DT_I32 : GHX_DT_I64) : (f.sp.elem == 4 ? GHX_DT_F32 : GHX_DT_F64));
    if (tile_bytes) CHECK(ghx_tune("tile_bytes", int64_t(tile_bytes)) == GHX_OK);
    const int rc = ghx_cs_exchange_adjoint_self_create(ex, dtypes.data(), int32_t(dtypes.size()));
    if (rc != GHX_OK) std::printf("c=%d %s self_create: %s\n", cfg.c, two_ranks ? "two ranks" : "one rank", ghx_last_error());
    if (tile_bytes) CHECK(ghx_tune("reset", 0) == GHX_OK);
    CHECK(rc == GHX_OK);
    int32_t form = -1;
    int64_t n_boxes = 0, n_sources = 0, n_fs = 0, n_rot = 0;
    CHECK(ghx_cs_exchange_adjoint_self_info(ex, &form, &n_boxes, &n_sources, &n_fs, &n_rot) == GHX_OK);
    CHECK(form == (two_ranks ? 2 : 1) && n_boxes > 0 && n_rot > 0);
    const exchange_plan::adjoint_set& set = ex->adjoint[exchange_plan::adj_cs_self];
    CHECK(bool(set.spack || set.xpack) == two_ranks);
    if (rc != GHX_OK || !set.saccum)
    {
        ghx_exchange_destroy(ex);
        return;
    }
    const saccum_plan& p = *set.saccum;
    CHECK(p.get && p.rotated);

    // the send buffers: what the peers' reverse packs would have delivered
    std::vector<std::vector<unsigned char>> sbuf;
    for (size_t b = 0; b < ex->send.size(); ++b)
        sbuf.emplace_back(size_t(ex->send[b].size), static_cast<unsigned char>(0));
    // small integers in every send entry's bytes, in its field's type
    for (const ghx_pack_entry& e : ex->entries[0])
    {
        const spec& s = fx.fields[size_t(e.field_slot)].sp;
        uint64_t n = 0;
        for (int b = 0; b < e.n_boxes; ++b)
        {
            uint64_t cells = uint64_t(s.nc);
            for (int d = 0; d < 3; ++d) cells *= uint64_t(e.boxes[b].last[d] - e.boxes[b].first[d] + 1);
            n += cells;
        }
        std::vector<unsigned char>& B = sbuf.at(size_t(e.buffer_slot));
        CHECK(e.buffer_offset + n * uint64_t(s.elem) <= B.size());
        for (uint64_t i = 0; i < n; ++i)
            store(s, B.data() + e.buffer_offset + i * uint64_t(s.elem), small((i << 8) + uint64_t(e.buffer_slot)));
    }

    // ------------------------------------------------------------------ the definition
    // which send buffers belong to self messages: those a receive buffer pairs with
    std::vector<char> self_send(ex->send.size(), 0);
    for (int i : ex->send_of_recv)
        if (i >= 0) self_send[size_t(i)] = 1;
    // per field and byte: is it a cell of a send box (owner), of a self message's receive box, of
    // a peer's receive box
    std::vector<std::vector<unsigned char>> owner, self_halo, peer_halo;
    for (const field& f : fx.fields)
    {
        owner.emplace_back(f.mem.size(), static_cast<unsigned char>(0));
        self_halo.emplace_back(f.mem.size(), static_cast<unsigned char>(0));
        peer_halo.emplace_back(f.mem.size(), static_cast<unsigned char>(0));
    }
    // peer contributions and owner cells from the send entries (ordinary boxes of the sender)
    for (const ghx_pack_entry& e : ex->entries[0])
    {
        field& f = fx.fields[size_t(e.field_slot)];
        uint64_t at = e.buffer_offset;
        for (int b = 0; b < e.n_boxes; ++b)
        {
            const dense_box box(f, e.boxes[b].first, e.boxes[b].last);
            for (int x = e.boxes[b].first[0]; x <= e.boxes[b].last[0]; ++x)
                for (int y = e.boxes[b].first[1]; y <= e.boxes[b].last[1]; ++y)
                    for (int z = e.boxes[b].first[2]; z <= e.boxes[b].last[2]; ++z)
                        for (int k = 0; k < f.sp.nc; ++k)
                        {
                            const int64_t off = f.offset(x, y, z, k);
                            CHECK(off >= 0 && size_t(off) + size_t(f.sp.elem) <= f.mem.size());
                            owner[size_t(e.field_slot)][size_t(off)] = 1;
                            if (self_send[size_t(e.buffer_slot)]) continue;
                            const int64_t loc = box.at({x - e.boxes[b].first[0], y - e.boxes[b].first[1],
                                                        z - e.boxes[b].first[2], k});
                            const int64_t v = load(f.sp, sbuf[size_t(e.buffer_slot)].data() + at + uint64_t(loc));
                            store(f.sp, f.want.data() + off, load(f.sp, f.want.data() + off) + v);
                        }
            at += uint64_t(box.bytes);
        }
    }
    // self contributions from the reference's geometry: halo cell h of field f goes to the cell
    // h.g of the sending domain's field of the same field set
    uint64_t n_self_cells = 0;
    bool self_space = false;
    int sender = -1;
    for_each_halo_cell(
        fx,
        [&](field&, const halo_entry& e, size_t) {
            sender = -1;
            for (size_t a = 0; a < fx.doms.size(); ++a)
                if (cs_domain_id(cfg.c, fx.doms[a]) == e.key.remote_id) sender = int(a);
            CHECK(sender >= 0);
            self_space = sender >= 0 && fx.doms[size_t(sender)].rank == 0;
            return true;
        },
        [&](field& f, const halo_entry&, size_t, const halo_cell& h) {
            const size_t fi = size_t(&f - fx.fields.data());
            const int64_t off = f.offset(h.x, h.y, h.z, h.k);
            if (!self_space)
            {
                ++peer_halo[fi][size_t(off)];
                return;
            }
            ++self_halo[fi][size_t(off)];
            ++n_self_cells;
            field& o = fx.fields[fi / n_mine * n_mine + size_t(sender)];
            const ghx_cs_domain& od = fx.doms[size_t(sender)];
            const int64_t to = o.offset(h.g[0] - od.x_first, h.g[1] - od.y_first, h.z, h.k);
            CHECK(to >= 0 && size_t(to) + size_t(o.sp.elem) <= o.mem.size());
            const int64_t v = load(f.sp, f.first.data() + off);
            store(o.sp, o.want.data() + to, load(o.sp, o.want.data() + to) + (h.neg ? -v : v));
        });
    CHECK(n_self_cells > 0);
    const std::vector<field> start = fx.fields;

    // ------------------------------------------------------------------ the replay
    for (int zero_halos = 0; zero_halos < 2; ++zero_halos)
        for (int narrow = 0; narrow < 3; ++narrow)
        {
            fx.fields = start;
            std::vector<std::vector<int>> reads, writes;
            for (const field& f : fx.fields)
            {
                reads.emplace_back(f.mem.size(), 0);
                writes.emplace_back(f.mem.size(), 0);
            }
            const size_t n_tiles = zero_halos ? p.tiles.size() : p.n_sum_tiles;
            for (size_t t = 0; t < n_tiles; ++t)
            {
                const sacc_tile& s = p.tiles[t];
                CHECK(size_t(s.field_slot) < fx.fields.size());
                field& f = fx.fields[s.field_slot];
                const int elem = f.sp.elem;
                int elog2 = elem == 8 ? 3 : 2;
                CHECK(s.wlog2 >= elog2 && s.wlog2 <= 4 && s.len % (1u << s.wlog2) == 0 && s.len > 0 && s.n_rows > 0);
                CHECK((t < p.n_sum_tiles) == (s.zero == 0) && (s.zero == 0) == (s.n_src > 0));
                CHECK(s.comp <= kSaccCompRow && s.pad == 0);
                if (s.comp == kSaccCompRow) CHECK(s.wlog2 == elog2);
                const int w = std::max(elog2, int(s.wlog2) - narrow);
                const uint32_t nv = sacc_vectors(s, w);
                CHECK(uint64_t(nv) << w == uint64_t(s.n_rows) * s.len);
                for (uint32_t i = 0; i < nv; ++i)
                {
                    uint32_t c[4], col;
                    sacc_decode(s, i, w, c, col);
                    CHECK(c[0] < s.ext[0] && c[1] < s.ext[1] && c[2] < s.ext[2] && c[3] < s.ext[3]);
                    CHECK(col >= s.col0 && col + (1u << w) <= s.col0 + s.len);
                    const int64_t foff = affine_offset(s.field_off, s.stride, c) + int64_t(col);
                    const bool in = fx.in_field(s.field_slot, foff, size_t(1) << w);
                    CHECK(in && foff % int64_t(1u << w) == 0);
                    if (!in) continue;
                    // the component of the lane's vector, as the kernel selects it
                    const uint32_t ci = s.comp == kSaccCompNone  ? 0u
                                        : s.comp == kSaccCompRow ? col / uint32_t(elem)
                                                                 : c[s.comp - 1];
                    const uint32_t sel = ci < 2u ? (1u << kSaccNegShift) << ci : 0u;
                    for (uint32_t k = 0; k < (1u << w) / uint32_t(elem); ++k)
                    {
                        const size_t at = size_t(foff) + size_t(k) * size_t(elem);
                        ++writes[s.field_slot][at];
                        if (s.zero)
                        {
                            store(f.sp, f.mem.data() + at, 0);
                            continue;
                        }
                        int64_t acc = load(f.sp, f.mem.data() + at);
                        for (uint32_t j = s.first_src; j < s.first_src + s.n_src; ++j)
                        {
                            const sacc_src& r = p.srcs.at(j);
                            CHECK(r.buf_slot < p.tab_slot.size() && ((s.buf_mask >> r.buf_slot) & 1u));
                            const bool from_field = (r.flags & kSaccFieldSrc) != 0;
                            CHECK(from_field == (r.buf_slot >= p.tab_field) && (r.flags >> 3) == 0);
                            if (!from_field) CHECK((r.flags >> kSaccNegShift) == 0);
                            const uint64_t uoff = r.buf_off + uint64_t(c[0]) * r.stride[0] + uint64_t(c[1]) * r.stride[1] +
                                                  uint64_t(c[2]) * r.stride[2] + uint64_t(c[3]) * r.stride[3] + col;
                            const int64_t off = int64_t(uoff) + int64_t(k) * elem;  // signed strides mod 2^64
                            CHECK(int64_t(uoff) % int64_t(1u << w) == 0);
                            const int32_t slot = p.tab_slot[r.buf_slot];
                            if (!from_field)
                            {
                                const std::vector<unsigned char>& B = sbuf.at(size_t(slot));
                                const bool ok = off >= 0 && size_t(off) + size_t(elem) <= B.size();
                                CHECK(ok);
                                if (ok) acc += load(f.sp, B.data() + off);
                                continue;
                            }
                            const bool ok = fx.in_field(slot, off, size_t(elem));
                            CHECK(ok);
                            if (!ok) continue;
                            field& g = fx.fields[size_t(slot)];
                            CHECK(++reads[size_t(slot)][size_t(off)] == 1);  // read once: the launch's input
                            const int64_t v = load(g.sp, g.mem.data() + off);
                            acc += (r.flags & sel) ? -v : v;
                            if (zero_halos) store(g.sp, g.mem.data() + off, 0);
                        }
                        store(f.sp, f.mem.data() + at, acc);
                    }
                }
            }
            for (size_t k = 0; k < fx.fields.size(); ++k)
            {
                const field& f = fx.fields[k];
                std::vector<unsigned char> want = f.want;
                for (size_t i = 0; zero_halos && i + size_t(f.sp.elem) <= want.size(); ++i)
                    if (self_halo[k][i] || peer_halo[k][i]) store(f.sp, want.data() + i, 0);
                for (size_t i = 0; i + size_t(f.sp.elem) <= f.mem.size(); i += size_t(f.sp.elem))
                    CHECK(load(f.sp, f.mem.data() + i) == load(f.sp, want.data() + i));
                for (size_t i = 0; i < f.mem.size(); ++i)
                {
                    CHECK(reads[k][i] == int(self_halo[k][i]));  // every source cell once, no other cell
                    if (owner[k][i]) CHECK(writes[k][i] == 1);   // every owner cell written once
                    else CHECK(writes[k][i] == ((zero_halos && peer_halo[k][i]) ? 1 : 0));
                }
            }
        }
    std::printf("c=%d levels=%d layout=%d%d%d%d fields=%zu (elem %d..) %s tile_bytes=%u: form %d, %lld sub-boxes, %lld sources, "
                "%lld rotated boxes, %zu tiles, %llu self halo cells\n",
                cfg.c, cfg.levels, layout[0], layout[1], layout[2], layout[3], specs.size(), specs[0].elem,
                two_ranks ? "two ranks" : "one rank", tile_bytes ? tile_bytes : 8192u, form, static_cast<long long>(n_boxes),
                static_cast<long long>(n_sources), static_cast<long long>(n_rot), p.tiles.size(),
                static_cast<unsigned long long>(n_self_cells));
    ghx_exchange_destroy(ex);
}
}  // namespace

int main()
{
    const config cfgs[] = {{6, 2, {1, 2, 0, 3}, 1, 1}, {8, 2, {2, 2, 2, 2}, 2, 1}, {10, 3, {2, 2, 2, 2}, 2, 2}, {70, 5, {3, 3, 3, 3}, 1, 1}};
    const int layouts[][4] = {{3, 2, 1, 0}, {2, 3, 1, 0}, {1, 2, 3, 0}, {0, 1, 2, 3}};
    for (const config& cfg : cfgs)
        for (const auto& layout : layouts)
            for (const bool two : {false, true})
                for (const uint32_t tb : {0u, 1024u})
                {
                    if (cfg.c == 70 && (tb || layout[0] == 2)) continue;  // the long rows once per form
                    // 12 of 24 domains on a rank: its peer messages' send buffers have slots past
                    // 64, which one accumulate launch refuses (tests/test_cs_get_host.py)
                    if (cfg.c == 10 && two) continue;
                    // an fp64 scalar and an f32 3-vector in one exchange; the 24-domain cube on one
                    // rank holds one field set more than 64 slots would
                    run(cfg, layout, {{8, 1, 0, 1}, {4, 3, 1, 1}}, two, tb);
                    if (cfg.c == 10 && !two) continue;
                    run(cfg, layout, {{8, 2, 1, 1}, {4, 2, 1, 2}, {8, 3, 1, 2}}, two, tb);
                }
    std::printf(g_fail ? "cs_get_host_check: %d FAILURES\n" : "cs_get_host_check: OK\n", g_fail);
    return g_fail ? 1 : 0;
}
