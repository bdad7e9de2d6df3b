// cs_adjoint_host_check — stand-alone host program (its own main; links the library's sources) for
// the reverse pack of the cubed-sphere adjoint exchange. It plans the cubed-sphere fixture
// geometries with all domains on one rank (ghx_cs_pattern_create, ghx_cs_exchange_create, no
// device), attaches the adjoint plans (exchange_plan::make_adjoint; the accumulate's 64-slot
// limit refuses the 24-domain geometry, whose reverse pack is replayed all the same) and replays
// on the host, with the kernels' own address arithmetic (ghx_addr.hpp) exactly as k_pack_x and
// k_copy<true, seg_s> index them, every seg_x tile record of the transformed unpack plan with the
// data direction reversed and every segment of the ordinary reverse pack, each field and buffer
// access bounds-checked. It checks that the tile records write every buffer byte of every
// transformed box exactly once, that both parts together write every payload byte of every
// receive buffer exactly once, that they read receive-box cells only, and that the buffers hold
// the transpose of the reference's rotating, negating unpack
// (cubed_sphere/field_descriptor.hpp:81-108): B[T(x, y), z, k] = s_k * R[x, y, z, k]. Elements of
// 1 to 16 bytes, both negations at 4 and 8 bytes, two fields of different width in one exchange,
// each at the default tile size and at x_tile_elems 32, 48 and 4096. Built with
// -fsanitize=address,undefined by tools/cs_host_sanitize.sh; needs no GPU.
#include "cs_check.hpp"

using namespace cs_check;

namespace
{
void run(const config& cfg, const int* layout, const std::vector<spec>& specs, int x_tile_elems)
{
    fixture fx(cfg, layout, specs);
    if (!fx.pat) return;
    std::vector<ghx_exchange_item> items;
    std::vector<ghx_cs_item> cs;
    fx.items(items, cs);
    // a planning knob: read when the exchange is created
    if (x_tile_elems) CHECK(ghx_tune("x_tile_elems", x_tile_elems) == GHX_OK);
    ghx_exchange* ex = nullptr;
    const int rc = ghx_cs_exchange_create(items.data(), cs.data(), int(items.size()), &ex);
    if (x_tile_elems) CHECK(ghx_tune("reset", 0) == GHX_OK);
    if (rc != GHX_OK) std::printf("create: %s\n", ghx_last_error());
    CHECK(rc == GHX_OK);
    if (!ex) return;

    // the adjoint plans, where the element type is one the accumulate sums
    bool summed = true;
    std::vector<int32_t> dtypes;
    for (const field& f : fx.fields)
    {
        const spec& s = f.sp;
        summed = summed && (s.elem == 4 || s.elem == 8);
        dtypes.push_back(s.kind == 2 ? (s.elem == 4 ? GHX_DT_I32 : GHX_DT_I64)
                                     : (s.elem == 4 ? GHX_DT_F32 : GHX_DT_F64));
    }
    const bool fits = ex->recv.size() <= size_t(GHX_MAX_SLOTS) && fx.fields.size() <= size_t(GHX_MAX_SLOTS);
    int32_t ready = -1, nxr = -1, nxt = -1;
    if (summed)
    {
        const int arc = ghx_cs_exchange_adjoint_create(ex, dtypes.data(), int32_t(dtypes.size()));
        CHECK((arc == GHX_OK) == fits);
        CHECK(ghx_cs_exchange_adjoint_info(ex, &ready, nullptr, nullptr, &nxr, &nxt) == GHX_OK);
        CHECK(ready == (fits ? 1 : 0));
        if (fits)
        {
            CHECK(nxr == (ex->xunpack ? ex->xunpack->n_records : 0));
            CHECK(nxt == (ex->xunpack ? int32_t(ex->xunpack->n_tiles) : 0));
            CHECK(bool(ex->adjoint[exchange_plan::adj_cs].spack) == bool(ex->sunpack));
        }
    }
    // the ordinary reverse pack of an exchange without adjoint plans: built as create builds it
    std::unique_ptr<splan> own_pack;
    const std::unique_ptr<splan>& adj_pack = ex->adjoint[exchange_plan::adj_cs].spack;
    if (!adj_pack && !ex->cs_segs.empty())
        own_pack = std::make_unique<splan>(ex->cs_segs, ex->cs_gf, ex->cs_gb, ex->cs_sbytes, 0);
    const splan* pack = adj_pack ? adj_pack.get() : own_pack.get();
    CHECK(bool(pack) == bool(ex->sunpack));
    if (pack && ex->sunpack) CHECK(pack->n_segments == ex->sunpack->n_segments && pack->bytes == ex->sunpack->bytes);

    // receive buffers: got (what the replay writes) and want (the transpose of the unpack)
    std::vector<std::vector<unsigned char>> got, want, bwritten, xbytes;
    for (size_t b = 0; b < ex->recv.size(); ++b)
    {
        got.emplace_back(size_t(ex->recv[b].size), static_cast<unsigned char>(0x5A));
        want.emplace_back(size_t(ex->recv[b].size), static_cast<unsigned char>(0x5A));
        bwritten.emplace_back(size_t(ex->recv[b].size), static_cast<unsigned char>(0));
        xbytes.emplace_back(size_t(ex->recv[b].size), static_cast<unsigned char>(0));
    }
    auto buf_write = [&](int slot, uint64_t off, const void* from, size_t n) {
        const bool ok = slot >= 0 && size_t(slot) < got.size() && off + n <= got[size_t(slot)].size();
        CHECK(ok);
        if (!ok) return;
        std::memcpy(got[size_t(slot)].data() + off, from, n);
        for (size_t i = 0; i < n; ++i) ++bwritten[size_t(slot)][size_t(off) + i];
    };
    auto caller = [](const std::vector<int32_t>& map, int local) {
        if (map.empty()) return local;
        CHECK(local >= 0 && size_t(local) < map.size());
        return local >= 0 && size_t(local) < map.size() ? int(map[size_t(local)]) : -1;
    };

    // ------------------------------------------------------------------ the transformed records
    uint64_t x_bytes = 0, s_bytes = 0;
    if (ex->xunpack)
    {
        for (const xseg& b : ex->xunpack->boxes)
        {
            const bool ok = b.buf_slot >= 0 && size_t(b.buf_slot) < xbytes.size() &&
                            b.buf_off + b.bytes() <= xbytes[size_t(b.buf_slot)].size();
            CHECK(ok);
            if (!ok) continue;
            for (uint64_t i = 0; i < b.bytes(); ++i) ++xbytes[size_t(b.buf_slot)][size_t(b.buf_off + i)];
        }
        for (const launch_group<seg_x>& g : ex->xunpack->groups)
            for (const seg_x& s : g.host_segs)
            {
                const size_t e = size_t(1) << s.elog2;
                const int fs = caller(g.fmap, s.field_slot), bs = caller(g.bmap, s.buf_slot);
                replay_tile(s, x_tile_elems, [&](const uint32_t (&c)[4], int64_t from) {
                    value v;
                    if (!fx.src_read(fs, from, &v, e)) return false;
                    v = stored_value(s, c, v);
                    buf_write(bs, s.buf_off + (uint64_t(tile_cell(s, c)) << s.elog2), &v, e);
                    return true;
                });
                x_bytes += s.bytes;
            }
        CHECK(x_bytes == ex->xunpack->bytes);
    }
    // every byte of every transformed box is written exactly once, by the records alone
    for (size_t k = 0; k < got.size(); ++k)
        for (size_t i = 0; i < got[k].size(); ++i)
        {
            CHECK(xbytes[k][i] <= 1);
            CHECK(bwritten[k][i] == xbytes[k][i]);
        }

    // ------------------------------------------------------------------ the ordinary reverse pack
    if (pack)
        for (const launch_group<seg_s>& g : pack->groups)
            for (const seg_s& s : g.host_segs)
            {
                const int fs = caller(g.fmap, s.field_slot), bs = caller(g.bmap, s.buf_slot);
                CHECK(s.row_bytes % (1u << s.wlog2) == 0);
                for (uint32_t p = 0; p < s.bytes; ++p)
                {
                    const int64_t fo = field_offset_s(s, p);
                    if (s.amode) CHECK(offset_f(s, p) == fo);
                    unsigned char v = 0;
                    if (!fx.src_read(fs, fo, &v, 1)) continue;
                    buf_write(bs, s.buf_off + p, &v, 1);
                }
                s_bytes += s.bytes;
            }

    // ------------------------------------------------------------------ the transpose of unpack
    std::map<std::pair<int32_t, int32_t>, uint64_t> fill;
    auto buffer_of = [&](int32_t first, int32_t second) {
        size_t b = 0;
        while (b < ex->recv.size() && !(ex->recv[b].first_id == first && ex->recv[b].second_id == second)) ++b;
        CHECK(b < ex->recv.size());
        return b;
    };
    std::vector<std::vector<unsigned char>> halo;  // per field: the bytes of its receive boxes
    for (const field& f : fx.fields) halo.emplace_back(f.mem.size(), static_cast<unsigned char>(0));
    size_t b = 0;
    uint64_t base = 0, payload = 0;
    const uint64_t cells = for_each_halo_cell(
        fx,
        [&](field& f, const halo_entry& e, size_t i) {
            const int32_t id = fx.pat->doms[size_t(f.dom)].id;
            b = buffer_of(id, e.key.remote_id);
            if (b >= ex->recv.size()) return false;
            uint64_t& at = fill[{id, e.key.remote_id}];
            const uint64_t elem = uint64_t(f.sp.elem);
            base = at = (at + elem - 1) / elem * elem;
            const dense_box box(f, e.boxes[i].gf, e.boxes[i].gl);
            CHECK(base + uint64_t(box.bytes) <= want[b].size());
            if (base + uint64_t(box.bytes) > want[b].size()) return false;
            at += uint64_t(box.bytes);
            payload += uint64_t(box.bytes);
            return true;
        },
        [&](field& f, const halo_entry& e, size_t i, const halo_cell& h) {
            const is_pair& bx = e.boxes[i];
            const dense_box box(f, bx.gf, bx.gl);
            const int64_t loc = box.at({h.g[0] - bx.gf[0], h.g[1] - bx.gf[1], h.z - bx.gf[2], h.k});
            const int64_t off = f.offset(h.x, h.y, h.z, h.k);
            value v;
            std::memcpy(&v, f.first.data() + off, size_t(f.sp.elem));
            if (h.neg) v = negated(v, f.sp.elem, f.sp.kind);
            std::memcpy(want[b].data() + base + uint64_t(loc), &v, size_t(f.sp.elem));
            const size_t fi = size_t(&f - fx.fields.data());
            for (int q = 0; q < f.sp.elem; ++q) ++halo[fi][size_t(off) + size_t(q)];
        });

    // ------------------------------------------------------------------ comparison
    CHECK(x_bytes + s_bytes == payload);
    for (size_t k = 0; k < got.size(); ++k)
    {
        CHECK(got[k] == want[k]);
        uint64_t more = 0;
        for (unsigned char w : bwritten[k]) more += w > 1;
        CHECK(more == 0);
    }
    // the field is read only: only receive-box cells, each exactly the bytes a box holds once
    uint64_t read_bytes = 0;
    for (size_t fi = 0; fi < fx.fields.size(); ++fi)
    {
        const field& f = fx.fields[fi];
        CHECK(f.mem == f.first);
        for (size_t i = 0; i < f.mem.size(); ++i)
        {
            CHECK(f.written[i] == 0);
            CHECK(halo[fi][i] <= 1);  // the receive boxes are disjoint
            CHECK(f.read[i] == halo[fi][i]);
            read_bytes += f.read[i];
        }
    }
    CHECK(read_bytes == payload);
    std::printf("c=%d levels=%d layout=%d%d%d%d fields=%zu (elem %d..) x_tile_elems=%d: %llu halo cells, "
                "%llu B in %u transformed tiles, %llu B in ordinary segments, adjoint plans %s\n",
                cfg.c, cfg.levels, layout[0], layout[1], layout[2], layout[3], specs.size(), specs[0].elem,
                x_tile_elems ? x_tile_elems : 256, static_cast<unsigned long long>(cells),
                static_cast<unsigned long long>(x_bytes), ex->xunpack ? ex->xunpack->n_tiles : 0u,
                static_cast<unsigned long long>(s_bytes),
                !summed ? "not asked (no summed type)" : fits ? "ready" : "refused (slots)");
    ghx_exchange_destroy(ex);
}
}  // namespace

int main()
{
    const config cfgs[] = {{10, 3, {2, 2, 2, 2}, 2, 2}, {6, 2, {1, 2, 0, 3}, 1, 1},
                           {70, 5, {3, 3, 3, 3}, 1, 1}, {8, 2, {2, 2, 2, 2}, 2, 1}};
    const int layouts[][4] = {{3, 2, 1, 0}, {2, 3, 1, 0}, {1, 2, 3, 0}, {0, 1, 2, 3}};
    for (const config& cfg : cfgs)
        for (const auto& layout : layouts)
            for (const int tile : {0, 32, 48, 4096})  // 0: the default, no knob set
            {
                // an fp64 scalar and an f32 3-vector in one exchange (two widths per buffer)
                run(cfg, layout, {{8, 1, 0, 1}, {4, 3, 1, 1}}, tile);
                run(cfg, layout, {{4, 3, 1, 2}}, tile);
                run(cfg, layout, {{8, 2, 1, 1}, {8, 3, 1, 2}}, tile);
                // the other widths (scalars: opaque bits)
                run(cfg, layout, {{1, 1, 0, 0}, {2, 3, 0, 0}}, tile);
                run(cfg, layout, {{16, 1, 0, 0}}, tile);
            }
    std::printf(g_fail ? "cs_adjoint_host_check: %d FAILURES\n" : "cs_adjoint_host_check: OK\n", g_fail);
    return g_fail ? 1 : 0;
}
