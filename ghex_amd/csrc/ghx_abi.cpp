// ghx_abi.cpp — the extern "C" boundary (include/ghx.h): argument checks, error capture and
// opaque handles. Every function checks its arguments and makes one call: the planners are in
// ghx_plan.cpp and ghx_exchange.cpp, the per-call entry points' plan caches in ghx_cache.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "ghx_cubed_sphere.hpp"
#include "ghx_exchange.hpp"
#include "ghx_guard.hpp"
#include "ghx_pattern.hpp"
#include "ghx_plan.hpp"

namespace ghx
{
namespace
{
thread_local std::string g_error;
}
void set_error(const std::string& msg) { g_error = msg; }
const char* get_error() { return g_error.c_str(); }

}  // namespace ghx

using namespace ghx;

namespace
{
int check_ptr(const void* p, const char* what)
{
    if (!p) throw invalid(std::string("null argument: ") + what);
    return 0;
}
}  // namespace

extern "C" {

const char* ghx_last_error(void) { return ghx::get_error(); }

const char* ghx_version(void) { return "ghex_amd 0.1.0 (gfx950)"; }

int ghx_tune(const char* key, int32_t value)
{
    // one row per knob: the member (an int or a uint32_t of `tuning`), the rule its values obey
    // (lo / hi: the range rules' bounds) and the refusal of every other value
    enum rule { flag, range, zero_or_range, pow2, zero_or_pow2 };  // pow2: in [1 KiB, 1 MiB]
    struct knob
    {
        const char* key;
        int tuning::*i;
        uint32_t tuning::*u;
        rule r;
        int32_t lo, hi;
        const char* refusal;
    };
    constexpr int32_t kMax = INT32_MAX;
    static const knob knobs[] = {
        {"order", &tuning::order, nullptr, flag, 0, 1, "order must be 0 or 1"},
        {"self_tile_bytes", nullptr, &tuning::self_tile_bytes, pow2, 0, 0,
         "self_tile_bytes must be a power of two in [1 KiB, 1 MiB]"},
        {"mixed_always", &tuning::mixed_always, nullptr, flag, 0, 1, "mixed_always must be 0 or 1"},
        {"unpack_tile_bytes", nullptr, &tuning::unpack_tile_bytes, zero_or_pow2, 0, 0,
         "unpack_tile_bytes must be 0 or a power of two in [1 KiB, 1 MiB]"},
        {"tile_records", &tuning::tile_records, nullptr, flag, 0, 1, "tile_records must be 0 or 1"},
        {"pack_tile_rows", nullptr, &tuning::pack_tile_rows, zero_or_range, 64, 65536,
         "pack_tile_rows must be 0 (as small_tile_rows) or in [64, 65536]"},
        {"unpack_tile_rows", nullptr, &tuning::unpack_tile_rows, zero_or_range, 64, 65536,
         "unpack_tile_rows must be 0 (as small_tile_rows) or in [64, 65536]"},
        {"fast_addr", &tuning::fast_addr, nullptr, flag, 0, 1, "fast_addr must be 0 or 1"},
        {"x_tile_elems", nullptr, &tuning::x_tile_elems, range, 32, 4096,
         "x_tile_elems must be in [32, 4096]"},
        {"xcd_pair", &tuning::xcd_pair, nullptr, flag, 0, 1, "xcd_pair must be 0 or 1"},
        {"u_tile_rows", nullptr, &tuning::u_tile_rows, range, 1, kMax, "u_tile_rows must be >= 1"},
        {"u_tile_bytes", nullptr, &tuning::u_tile_bytes, pow2, 0, 0,
         "u_tile_bytes must be a power of two in [1 KiB, 1 MiB]"},
        {"urun", &tuning::urun, nullptr, flag, 0, 1, "urun must be 0 or 1"},
        {"u_run_tile_rows", nullptr, &tuning::u_run_tile_rows, range, 4, kMax,
         "u_run_tile_rows must be >= 4"},
        {"short_pol", &tuning::short_pol, nullptr, range, 0, 3, "short_pol must be in 0..3"},
        {"small_row_bytes", nullptr, &tuning::small_row_bytes, range, 1, kMax,
         "small_row_bytes must be >= 1"},
        {"small_tile_rows", nullptr, &tuning::small_tile_rows, zero_or_range, 64, 65536,
         "small_tile_rows must be 0 (auto) or in [64, 65536]"},
        {"grid_cap", &tuning::grid_cap, nullptr, range, 0, kMax, "grid_cap must be >= 0"},
        {"tile_bytes", nullptr, &tuning::tile_bytes, pow2, 0, 0,
         "tile_bytes must be a power of two in [1 KiB, 1 MiB]"},
    };
    return guarded([&] {
        check_ptr(key, "key");
        const std::string k(key);
        if (k == "reset")
        {
            g_tune = tuning{};
            return GHX_OK;
        }
        for (const knob& kn : knobs)
        {
            if (k != kn.key) continue;
            bool ok;
            if (kn.r == pow2 || kn.r == zero_or_pow2)
                ok = value >= 1024 && uint32_t(value) <= kMaxTileBytes && !(value & (value - 1));
            else ok = value >= kn.lo && value <= kn.hi;
            if (value == 0 && (kn.r == zero_or_range || kn.r == zero_or_pow2)) ok = true;
            if (!ok) throw invalid(kn.refusal);
            if (kn.i) g_tune.*kn.i = value;
            else g_tune.*kn.u = uint32_t(value);
            return GHX_OK;
        }
        throw invalid("unknown tuning key: " + k);
    });
}

int ghx_launch_timing(int32_t enable)
{
    return guarded([&] {
        ghx::timing_enable(enable != 0);
        return GHX_OK;
    });
}

int ghx_launch_timing_read(float* ms, int32_t cap, int32_t* n)
{
    return guarded([&] {
        if (cap < 0 || (cap > 0 && !ms)) throw invalid("bad ms / cap");
        return ghx::timing_read(ms, cap, n);
    });
}

int ghx_plan_create(const ghx_pack_entry* entries, int32_t n_entries, int32_t direction,
                    ghx_plan** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        if (n_entries < 0 || (n_entries > 0 && !entries)) throw invalid("bad entries");
        *out = new ghx_plan(entries, n_entries, direction);
        return GHX_OK;
    });
}

int ghx_plan_execute(const ghx_plan* plan, void* const* field_ptrs, int32_t n_field_ptrs,
                     void* const* buffer_ptrs, int32_t n_buffer_ptrs, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(plan, "plan");
        return plan->execute(field_ptrs, n_field_ptrs, buffer_ptrs, n_buffer_ptrs, stream);
    });
}

int ghx_plan_destroy(ghx_plan* plan)
{
    return guarded([&] {
        delete plan;
        return GHX_OK;
    });
}

int ghx_plan_info(const ghx_plan* plan, uint64_t* bytes, int32_t* n_segments, int32_t* n_tiles)
{
    return guarded([&] {
        check_ptr(plan, "plan");
        if (bytes) *bytes = plan->bytes;
        if (n_segments) *n_segments = plan->n_segments;
        if (n_tiles) *n_tiles = int32_t(plan->total_tiles());
        return GHX_OK;
    });
}

int ghx_plan_segment(const ghx_plan* plan, int32_t k, ghx_segment_info* out)
{
    return guarded([&] {
        check_ptr(plan, "plan");
        check_ptr(out, "out");
        if (k < 0 || k >= plan->n_segments) throw invalid("segment index out of range");
        // the host copies of the launch groups, in plan order (partition_slots keeps it)
        size_t i = size_t(k), g = 0;
        while (g < plan->groups.size() && i >= plan->groups[g].host_segs.size())
            i -= plan->groups[g++].host_segs.size();
        if (g == plan->groups.size()) throw invalid("segment index out of range");
        const launch_group<seg_s>& grp = plan->groups[g];
        const seg_s& s = grp.host_segs[i];
        *out = ghx_segment_info{};
        out->field_off = s.field_off;
        out->buf_off = s.buf_off;
        for (int d = 0; d < 4; ++d)
        {
            out->stride[d] = s.stride[d];
            out->ext[d] = s.ext[d];
        }
        out->row_bytes = s.row_bytes;
        out->bytes = s.bytes;
        out->tile_bytes = s.tile_bytes;
        out->field_slot = grp.fmap.empty() ? int32_t(s.field_slot) : grp.fmap[s.field_slot];
        out->buffer_slot = grp.bmap.empty() ? int32_t(s.buf_slot) : grp.bmap[s.buf_slot];
        out->n_outer = s.n_outer;
        out->wlog2 = s.wlog2;
        out->amode = s.amode;
        out->pipe = s.pipe;
        return GHX_OK;
    });
}

int ghx_structured_pack(const ghx_field_desc* field, const void* field_data, void* buffer,
                        const ghx_box* boxes, int32_t n_boxes, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(field, "field");
        if (n_boxes < 0 || (n_boxes > 0 && !boxes)) throw invalid("bad boxes");
        return run_structured(*field, boxes, n_boxes, 0, const_cast<void*>(field_data), buffer,
                              stream);
    });
}

int ghx_structured_unpack(const ghx_field_desc* field, void* field_data, const void* buffer,
                          const ghx_box* boxes, int32_t n_boxes, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(field, "field");
        if (n_boxes < 0 || (n_boxes > 0 && !boxes)) throw invalid("bad boxes");
        return run_structured(*field, boxes, n_boxes, 1, field_data, const_cast<void*>(buffer),
                              stream);
    });
}

int ghx_unstructured_pack(const ghx_udata_desc* data, const void* values, void* buffer,
                          const void* lids, int32_t lid_bytes, int64_t n_lids, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(data, "data");
        if (lid_bytes != 4 && lid_bytes != 8) throw invalid("lid_bytes must be 4 or 8");
        if (n_lids < 0 || (n_lids > 0 && !lids)) throw invalid("bad index list");
        if (n_lids == 0) return int(GHX_OK);
        return run_unstructured(*data, lids, lid_bytes, n_lids, 0, const_cast<void*>(values),
                                buffer, stream);
    });
}

int ghx_unstructured_unpack(const ghx_udata_desc* data, void* values, const void* buffer,
                            const void* lids, int32_t lid_bytes, int64_t n_lids, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(data, "data");
        if (lid_bytes != 4 && lid_bytes != 8) throw invalid("lid_bytes must be 4 or 8");
        if (n_lids < 0 || (n_lids > 0 && !lids)) throw invalid("bad index list");
        if (n_lids == 0) return int(GHX_OK);
        return run_unstructured(*data, lids, lid_bytes, n_lids, 1, values,
                                const_cast<void*>(buffer), stream);
    });
}

int ghx_uplan_create(const ghx_upack_entry* entries, int32_t n_entries, int32_t direction,
                     ghx_uplan** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        if (n_entries < 0 || (n_entries > 0 && !entries)) throw invalid("bad entries");
        *out = new ghx_uplan(entries, n_entries, direction);
        return GHX_OK;
    });
}

int ghx_uplan_execute(const ghx_uplan* plan, void* const* field_ptrs, int32_t n_field_ptrs,
                      void* const* buffer_ptrs, int32_t n_buffer_ptrs, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(plan, "plan");
        return plan->execute(field_ptrs, n_field_ptrs, buffer_ptrs, n_buffer_ptrs, stream);
    });
}

int ghx_uplan_destroy(ghx_uplan* plan)
{
    return guarded([&] {
        delete plan;
        return GHX_OK;
    });
}

int ghx_uplan_info(const ghx_uplan* plan, uint64_t* bytes, int32_t* n_segments, int32_t* n_tiles)
{
    return guarded([&] {
        check_ptr(plan, "plan");
        if (bytes) *bytes = plan->bytes;
        if (n_segments) *n_segments = plan->n_segments;
        if (n_tiles) *n_tiles = int32_t(plan->total_tiles());
        return GHX_OK;
    });
}

namespace
{
// segment k of an index-list plan (ghx_uplan_segment, ghx_umixed_peer_segment)
void usegment_info(const uplan* plan, int32_t k, ghx_usegment_info* out)
{
    if (k < 0 || k >= plan->n_segments) throw invalid("segment index out of range");
    // the host copies of the launch groups, in plan order (as ghx_plan_segment)
    size_t i = size_t(k), g = 0;
    while (g < plan->groups.size() && i >= plan->groups[g].host_segs.size())
        i -= plan->groups[g++].host_segs.size();
    if (g == plan->groups.size()) throw invalid("segment index out of range");
    const launch_group<seg_u>& grp = plan->groups[g];
    const seg_u& s = grp.host_segs[i];
    *out = ghx_usegment_info{};
    out->field_off = s.field_off;
    out->buf_off = s.buf_off;
    out->index_stride_b = s.index_stride_b;
    out->level_stride_b = s.level_stride_b;
    out->bytes = s.bytes;
    out->row_bytes = s.row_bytes;
    out->tile_bytes = s.tile_bytes;
    out->n = s.n;
    out->field_slot = grp.fmap.empty() ? int32_t(s.field_slot) : grp.fmap[s.field_slot];
    out->buffer_slot = grp.bmap.empty() ? int32_t(s.buf_slot) : grp.bmap[s.buf_slot];
    out->mode = s.mode;
    out->wlog2 = s.wlog2;
    out->lid64 = s.lid64;
    out->runs = s.runs;
    out->fpol = s.fpol;
}
}  // namespace

int ghx_uplan_segment(const ghx_uplan* plan, int32_t k, ghx_usegment_info* out)
{
    return guarded([&] {
        check_ptr(plan, "plan");
        check_ptr(out, "out");
        usegment_info(plan, k, out);
        return GHX_OK;
    });
}

// ----------------------------------------------------------------------------------- patterns
int ghx_regular_halo_boxes(int32_t dim, const int32_t* global_first, const int32_t* global_last,
                           const int32_t* halos, const int32_t* periodic,
                           const int32_t* domain_first, const int32_t* domain_last,
                           ghx_box* local, ghx_box* global, int32_t max_boxes, int32_t* n_boxes)
{
    return guarded([&] {
        if (dim < 1 || dim > 3) throw invalid("dim must be 1, 2 or 3");
        check_ptr(global_first, "global_first");
        check_ptr(global_last, "global_last");
        check_ptr(halos, "halos");
        check_ptr(periodic, "periodic");
        check_ptr(domain_first, "domain_first");
        check_ptr(domain_last, "domain_last");
        check_ptr(n_boxes, "n_boxes");
        auto b = regular_halo_boxes(dim, global_first, global_last, halos, periodic, domain_first,
                                    domain_last);
        *n_boxes = int32_t(b.size());
        for (int32_t i = 0; i < std::min<int32_t>(max_boxes, int32_t(b.size())); ++i)
        {
            ghx_box l{}, g{};
            for (int d = 0; d < dim; ++d)
            {
                l.first[d] = b[i].lf[d];
                l.last[d] = b[i].ll[d];
                g.first[d] = b[i].gf[d];
                g.last[d] = b[i].gl[d];
            }
            if (local) local[i] = l;
            if (global) global[i] = g;
        }
        return GHX_OK;
    });
}

int ghx_regular_pattern_create(int32_t dim, const ghx_regular_domain* domains,
                               int32_t n_domains, const int32_t* global_first,
                               const int32_t* global_last, const int32_t* halos,
                               const int32_t* periodic, int32_t my_rank, ghx_pattern** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        check_ptr(domains, "domains");
        check_ptr(global_first, "global_first");
        check_ptr(global_last, "global_last");
        check_ptr(halos, "halos");
        check_ptr(periodic, "periodic");
        if (dim < 1 || dim > 3) throw invalid("dim must be 1, 2 or 3");
        if (n_domains < 1) throw invalid("need at least one domain");
        for (int i = 0; i < n_domains; ++i)
            for (int j = 0; j < i; ++j)
                if (domains[i].id == domains[j].id) throw invalid("domain ids must be unique");
        auto p = std::make_unique<ghx_pattern>();
        regular_make_pattern(dim, domains, n_domains, global_first, global_last, halos, periodic,
                             my_rank, *p);
        *out = p.release();
        return GHX_OK;
    });
}

int ghx_staged_pattern_create(int32_t dim, const ghx_regular_domain* domains, int32_t n_domains,
                              const int32_t* neighbors, const int32_t* global_first,
                              const int32_t* global_last, const int32_t* halos,
                              const int32_t* periodic, int32_t my_rank, ghx_pattern** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        check_ptr(domains, "domains");
        check_ptr(neighbors, "neighbors");
        check_ptr(global_first, "global_first");
        check_ptr(global_last, "global_last");
        check_ptr(halos, "halos");
        check_ptr(periodic, "periodic");
        if (dim < 1 || dim > 3) throw invalid("dim must be 1, 2 or 3");
        if (n_domains < 1) throw invalid("need at least one domain");
        std::vector<ghx::pattern_set> sets;
        try
        {
            ghx::staged_make_pattern(dim, domains, n_domains, neighbors, global_first,
                                     global_last, halos, periodic, my_rank, sets);
        }
        catch (const std::runtime_error& e)
        {
            throw invalid(e.what());
        }
        std::vector<std::unique_ptr<ghx_pattern>> ps;
        for (auto& s : sets)
        {
            ps.push_back(std::make_unique<ghx_pattern>());
            static_cast<ghx::pattern_set&>(*ps.back()) = std::move(s);
        }
        for (int i = 0; i < dim; ++i) out[i] = ps[i].release();
        return GHX_OK;
    });
}

static const ghx::halo_entry& key_of(const ghx_pattern* p, int32_t li, int32_t dir, int32_t key);

int ghx_cs_halo_boxes(int32_t edge_size, int32_t levels, const ghx_cs_domain* domain,
                      const int32_t* halos, ghx_box* local, ghx_box* global, int32_t* tiles,
                      int32_t max_boxes, int32_t* n_boxes)
{
    return guarded([&] {
        check_ptr(domain, "domain");
        check_ptr(halos, "halos");
        check_ptr(n_boxes, "n_boxes");
        const auto b = cs_halo_boxes(edge_size, levels, *domain, halos);
        *n_boxes = int32_t(b.size());
        for (int32_t i = 0; i < std::min<int32_t>(max_boxes, int32_t(b.size())); ++i)
        {
            ghx_box l{}, g{};
            for (int d = 0; d < 3; ++d)
            {
                l.first[d] = b[size_t(i)].b.lf[d];
                l.last[d] = b[size_t(i)].b.ll[d];
                g.first[d] = b[size_t(i)].b.gf[d];
                g.last[d] = b[size_t(i)].b.gl[d];
            }
            if (local) local[i] = l;
            if (global) global[i] = g;
            if (tiles) tiles[i] = b[size_t(i)].tile;
        }
        return GHX_OK;
    });
}

int ghx_cs_pattern_create(int32_t edge_size, int32_t levels, const ghx_cs_domain* domains,
                          int32_t n_domains, const int32_t* halos, int32_t my_rank,
                          ghx_pattern** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        check_ptr(domains, "domains");
        check_ptr(halos, "halos");
        if (n_domains < 1) throw invalid("need at least one domain");
        auto p = std::make_unique<ghx_pattern>();
        cs_make_pattern(edge_size, levels, domains, n_domains, halos, my_rank, *p);
        *out = p.release();
        return GHX_OK;
    });
}

int ghx_pattern_key_tiles(const ghx_pattern* p, int32_t local_index, int32_t direction,
                          int32_t key, int32_t* tiles, int32_t max_boxes)
{
    return guarded([&] {
        const auto& e = key_of(p, local_index, direction, key);
        if (p->kind != 0 || p->cs_edge == 0) throw invalid("not a cubed-sphere pattern");
        check_ptr(tiles, "tiles");
        for (int32_t i = 0; i < std::min<int32_t>(max_boxes, int32_t(e.tiles.size())); ++i)
            tiles[i] = e.tiles[size_t(i)];
        return GHX_OK;
    });
}

int ghx_cs_unpack(const ghx_field_desc* field, const ghx_cs_item* cs, void* field_data,
                  const void* buffer, const ghx_box* local, const ghx_box* global,
                  const int32_t* tiles, int32_t n_boxes, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(field, "field");
        check_ptr(cs, "cs");
        if (n_boxes < 0 || (n_boxes > 0 && (!local || !global || !tiles))) throw invalid("bad boxes");
        check_cs_item(*field, *cs);
        if (n_boxes == 0) return int(GHX_OK);
        return run_cs_unpack(*field, *cs, local, global, tiles, n_boxes, field_data,
                             const_cast<void*>(buffer), stream);
    });
}

int ghx_cs_pack_rotated(const ghx_field_desc* field, const ghx_cs_item* cs, const void* field_data,
                        void* buffer, const ghx_box* local, const ghx_box* global,
                        const int32_t* tiles, int32_t n_boxes, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(field, "field");
        check_ptr(cs, "cs");
        if (n_boxes < 0 || (n_boxes > 0 && (!local || !global || !tiles))) throw invalid("bad boxes");
        check_cs_item(*field, *cs);
        if (n_boxes == 0) return int(GHX_OK);
        return run_cs_pack_rotated(*field, *cs, local, global, tiles, n_boxes, field_data, buffer, stream);
    });
}

int ghx_pattern_filter(const ghx_pattern* p, const int32_t* ranks, int32_t n_ranks, int32_t keep,
                       ghx_pattern** out)
{
    return guarded([&] {
        check_ptr(p, "pattern");
        check_ptr(out, "out");
        if (n_ranks < 0 || (n_ranks > 0 && !ranks)) throw invalid("bad rank list");
        if (keep != 0 && keep != 1) throw invalid("keep must be 0 or 1");
        auto in_set = [&](int32_t r) {
            for (int32_t i = 0; i < n_ranks; ++i)
                if (ranks[i] == r) return true;
            return false;
        };
        auto q = std::make_unique<ghx_pattern>();
        static_cast<pattern_set&>(*q) = static_cast<const pattern_set&>(*p);
        for (auto& d : q->doms)
            for (auto* v : {&d.send, &d.recv})
            {
                std::vector<halo_entry> kept;
                for (auto& e : *v)
                    if (in_set(e.key.remote_rank) == (keep == 1)) kept.push_back(std::move(e));
                v->swap(kept);
            }
        *out = q.release();
        return GHX_OK;
    });
}

int ghx_pattern_destroy(ghx_pattern* p)
{
    return guarded([&] {
        delete p;
        return GHX_OK;
    });
}

int ghx_pattern_num_domains(const ghx_pattern* p, int32_t* n)
{
    return guarded([&] {
        check_ptr(p, "pattern");
        check_ptr(n, "n");
        *n = int32_t(p->doms.size());
        return GHX_OK;
    });
}

int ghx_pattern_max_tag(const ghx_pattern* p, int32_t* max_tag)
{
    return guarded([&] {
        check_ptr(p, "pattern");
        check_ptr(max_tag, "max_tag");
        *max_tag = p->max_tag;
        return GHX_OK;
    });
}

int ghx_pattern_domain_id(const ghx_pattern* p, int32_t local_index, int32_t* id)
{
    return guarded([&] {
        check_ptr(p, "pattern");
        check_ptr(id, "id");
        if (local_index < 0 || local_index >= int32_t(p->doms.size())) throw invalid("local_index");
        *id = p->doms[size_t(local_index)].id;
        return GHX_OK;
    });
}

static const ghx::halo_entry& key_of(const ghx_pattern* p, int32_t li, int32_t dir, int32_t key)
{
    if (!p) throw invalid("null pattern");
    if (li < 0 || li >= int32_t(p->doms.size())) throw invalid("local_index out of range");
    const auto& v = dir == 0 ? p->doms[size_t(li)].send : p->doms[size_t(li)].recv;
    if (key < 0 || key >= int32_t(v.size())) throw invalid("key out of range");
    return v[size_t(key)];
}

int ghx_pattern_num_keys(const ghx_pattern* p, int32_t local_index, int32_t direction,
                         int32_t* n_keys)
{
    return guarded([&] {
        check_ptr(p, "pattern");
        check_ptr(n_keys, "n_keys");
        if (local_index < 0 || local_index >= int32_t(p->doms.size())) throw invalid("local_index");
        const auto& d = p->doms[size_t(local_index)];
        *n_keys = int32_t(direction == 0 ? d.send.size() : d.recv.size());
        return GHX_OK;
    });
}

int ghx_pattern_key(const ghx_pattern* p, int32_t local_index, int32_t direction, int32_t key,
                    int32_t* remote_id, int32_t* remote_rank, int32_t* tag, int32_t* n_spaces,
                    int64_t* n_elements)
{
    return guarded([&] {
        const auto& e = key_of(p, local_index, direction, key);
        if (remote_id) *remote_id = e.key.remote_id;
        if (remote_rank) *remote_rank = e.key.remote_rank;
        if (tag) *tag = e.key.tag;
        if (p->kind == 0)
        {
            if (n_spaces) *n_spaces = int32_t(e.boxes.size());
            if (n_elements)
            {
                int64_t n = 0;
                for (const auto& b : e.boxes) n += b.size(p->dim);
                *n_elements = n;
            }
        }
        else
        {
            if (n_spaces) *n_spaces = 1;
            if (n_elements) *n_elements = int64_t(e.lids.size());
        }
        return GHX_OK;
    });
}

int ghx_pattern_key_boxes(const ghx_pattern* p, int32_t local_index, int32_t direction,
                          int32_t key, ghx_box* local, ghx_box* global, int32_t max_boxes)
{
    return guarded([&] {
        const auto& e = key_of(p, local_index, direction, key);
        if (p->kind != 0) throw invalid("not a structured pattern");
        for (int32_t i = 0; i < std::min<int32_t>(max_boxes, int32_t(e.boxes.size())); ++i)
        {
            ghx_box l{}, g{};
            for (int d = 0; d < p->dim; ++d)
            {
                l.first[d] = e.boxes[size_t(i)].lf[d];
                l.last[d] = e.boxes[size_t(i)].ll[d];
                g.first[d] = e.boxes[size_t(i)].gf[d];
                g.last[d] = e.boxes[size_t(i)].gl[d];
            }
            if (local) local[i] = l;
            if (global) global[i] = g;
        }
        return GHX_OK;
    });
}

int ghx_pattern_key_lids(const ghx_pattern* p, int32_t local_index, int32_t direction,
                         int32_t key, int64_t* lids, int64_t max_lids)
{
    return guarded([&] {
        const auto& e = key_of(p, local_index, direction, key);
        if (p->kind != 1) throw invalid("not an unstructured pattern");
        check_ptr(lids, "lids");
        const int64_t n = std::min<int64_t>(max_lids, int64_t(e.lids.size()));
        std::memcpy(lids, e.lids.data(), size_t(n) * sizeof(int64_t));
        return GHX_OK;
    });
}

int ghx_exchange_create(const ghx_exchange_item* items, int32_t n_items, ghx_exchange** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = make_exchange(items, nullptr, n_items).release();
        return GHX_OK;
    });
}

int ghx_cs_exchange_create(const ghx_exchange_item* items, const ghx_cs_item* cs_items,
                           int32_t n_items, ghx_exchange** out)
{
    return guarded([&] {
        check_ptr(cs_items, "cs_items");
        if (n_items < 1 || !items) throw invalid("need at least one exchange item");
        for (int32_t i = 0; i < n_items; ++i)
        {
            if (items[i].kind != 0) throw invalid("cubed-sphere exchange items are structured fields");
            if (!items[i].pattern || items[i].pattern->cs_edge == 0)
                throw invalid("cubed-sphere exchange item whose pattern is not a cubed-sphere pattern");
            if (items[i].pattern->cs_edge != cs_items[i].edge_size)
                throw invalid("cubed-sphere exchange item: edge_size differs from the pattern's");
            check_cs_item(items[i].field, cs_items[i]);
        }
        check_ptr(out, "out");
        *out = make_exchange(items, cs_items, n_items).release();
        return GHX_OK;
    });
}

int ghx_cs_plan_info(const ghx_exchange* ex, int32_t* n_records, uint64_t* bytes,
                     int32_t* n_tiles, int32_t* n_rotated)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (n_records) *n_records = ex->xunpack ? ex->xunpack->n_records : 0;
        if (bytes) *bytes = ex->xunpack ? ex->xunpack->bytes : 0;
        if (n_tiles) *n_tiles = ex->xunpack ? int32_t(ex->xunpack->n_tiles) : 0;
        if (n_rotated) *n_rotated = ex->cs_rotated;
        return GHX_OK;
    });
}

int ghx_cs_self_info(const ghx_exchange* ex, int32_t* fusable, int32_t* n_pair_tiles,
                     int32_t* n_x_records, int32_t* n_x_tiles)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(fusable, "fusable");
        const cs_self_plan* p = ex->cs_self.get();
        *fusable = p ? 1 : 0;
        if (n_pair_tiles) *n_pair_tiles = p ? int32_t(p->n_pair_tiles()) : 0;
        if (n_x_records) *n_x_records = p ? p->n_x_records : 0;
        if (n_x_tiles) *n_x_tiles = p ? int32_t(p->n_x_tiles()) : 0;
        if (!p) set_error(ex->cs_self_reason);
        return GHX_OK;
    });
}

int ghx_cs_exchange_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                         void* const* buffers, int32_t n_buffers, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (!ex->cs_self) throw invalid("cubed-sphere self exchange: " + ex->cs_self_reason);
        if (ex->dir_parity[0].word)
            throw invalid("cubed-sphere self exchange: the send side has double-buffered buffers "
                          "(ghx_exchange_set_parity); the fused launch writes one copy");
        check_ptr(field_ptrs, "field_ptrs");
        check_ptr(buffers, "buffers");
        return ex->cs_self->execute(field_ptrs, n_fields, buffers, n_buffers, stream);
    });
}

int ghx_exchange_destroy(ghx_exchange* ex)
{
    return guarded([&] {
        delete ex;
        return GHX_OK;
    });
}

int ghx_exchange_num_buffers(const ghx_exchange* ex, int32_t direction, int32_t* n)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(n, "n");
        *n = int32_t(direction == 0 ? ex->send.size() : ex->recv.size());
        return GHX_OK;
    });
}

int ghx_exchange_buffer(const ghx_exchange* ex, int32_t direction, int32_t index,
                        int32_t* first_id, int32_t* second_id, int32_t* rank, int32_t* tag,
                        uint64_t* size)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        const auto& v = direction == 0 ? ex->send : ex->recv;
        if (index < 0 || index >= int32_t(v.size())) throw invalid("buffer index out of range");
        const auto& b = v[size_t(index)];
        if (first_id) *first_id = b.first_id;
        if (second_id) *second_id = b.second_id;
        if (rank) *rank = b.rank;
        if (tag) *tag = b.tag;
        if (size) *size = b.size;
        return GHX_OK;
    });
}

int ghx_exchange_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                      void* const* send_buffers, int32_t n_send, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (n_send < int32_t(ex->send.size())) throw invalid("too few send buffers");
        int rc = GHX_OK;
        if (ex->spack) rc = ex->spack->execute(field_ptrs, n_fields, send_buffers, n_send, stream);
        if (rc == GHX_OK && ex->upack)
            rc = ex->upack->execute(field_ptrs, n_fields, send_buffers, n_send, stream);
        return rc;
    });
}

int ghx_exchange_unpack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                        void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (n_recv < int32_t(ex->recv.size())) throw invalid("too few recv buffers");
        int rc = GHX_OK;
        if (ex->sunpack) rc = ex->sunpack->execute(field_ptrs, n_fields, recv_buffers, n_recv, stream);
        if (rc == GHX_OK && ex->uunpack)
            rc = ex->uunpack->execute(field_ptrs, n_fields, recv_buffers, n_recv, stream);
        // cubed sphere: the transformed spaces, after the ordinary launch on the same stream
        if (rc == GHX_OK && ex->xunpack)
            rc = ex->xunpack->execute(field_ptrs, n_fields, recv_buffers, n_recv, stream);
        return rc;
    });
}

int ghx_exchange_split(ghx_exchange* ex)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        ex->make_split();
        return GHX_OK;
    });
}

int ghx_exchange_pack_buffer(const ghx_exchange* ex, int32_t index, void* const* field_ptrs,
                             int32_t n_fields, void* const* send_buffers, int32_t n_send,
                             ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        return ex->execute_buffer(0, index, field_ptrs, n_fields, send_buffers, n_send, stream);
    });
}

int ghx_exchange_unpack_buffer(const ghx_exchange* ex, int32_t index, void* const* field_ptrs,
                               int32_t n_fields, void* const* recv_buffers, int32_t n_recv,
                               ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        return ex->execute_buffer(1, index, field_ptrs, n_fields, recv_buffers, n_recv, stream);
    });
}

int ghx_exchange_self_fusable(const ghx_exchange* ex, int32_t* fusable)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(fusable, "fusable");
        *fusable = ex->self_fusable() ? 1 : 0;
        return GHX_OK;
    });
}

int ghx_exchange_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                      void* const* buffers, int32_t n_buffers, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (!ex->self_fusable())
            throw invalid("exchange is not an all-self exchange with matching segments");
        return ex->execute_self(field_ptrs, n_fields, buffers, n_buffers, stream);
    });
}

int ghx_exchange_mixed(const ghx_exchange* ex, int32_t* mixed)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(mixed, "mixed");
        *mixed = ex->mixed ? 1 : 0;
        return GHX_OK;
    });
}

int ghx_exchange_pack_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                           void* const* send_buffers, int32_t n_send, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (!ex->mixed) throw invalid("exchange has no mixed self/peer plan (ghx_exchange_mixed)");
        if (n_send < int32_t(ex->send.size())) throw invalid("too few send buffers");
        return ex->execute_pack_self(field_ptrs, n_fields, send_buffers, n_send, stream);
    });
}

int ghx_exchange_set_parity(ghx_exchange* ex, int32_t direction, const uint64_t* parity_word,
                            uint32_t parity_add, const int64_t* offsets, int32_t n_buffers)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (direction != 0 && direction != 1) throw invalid("direction must be 0 (pack) or 1 (unpack)");
        if (direction == 1 && parity_word && ex->cs_rotated > 0)
            throw invalid("double-buffered receive buffers are not available on a cubed-sphere "
                          "exchange with rotated spaces (the transformed unpack reads one copy)");
        const size_t n = direction == 0 ? ex->send.size() : ex->recv.size();
        parity_cfg cfg;
        if (parity_word)
        {
            if (n_buffers != int32_t(n) || (n && !offsets))
                throw invalid("one offset per buffer of that direction");
            cfg.word = parity_word;
            cfg.add = parity_add & 1u;
            cfg.offset.assign(offsets, offsets + n);
            for (int64_t o : cfg.offset)
                if (o < 0 || o % 256 != 0)
                    throw invalid("second-copy offsets must be >= 0 and multiples of 256 B");
        }
        if (direction == 0)
        {
            if (ex->spack) ex->spack->parity = cfg;
            if (ex->upack) ex->upack->parity = cfg;
            ex->mixed_parity = cfg;
        }
        else
        {
            if (ex->sunpack) ex->sunpack->parity = cfg;
            if (ex->uunpack) ex->uunpack->parity = cfg;
            if (ex->punpack) ex->punpack->parity = cfg;
        }
        ex->dir_parity[direction] = cfg;
        if (ex->split) ex->set_split_parity(direction);
        return GHX_OK;
    });
}

int ghx_exchange_unpack_peers(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                              void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (!ex->mixed) throw invalid("exchange has no mixed self/peer plan (ghx_exchange_mixed)");
        if (n_recv < int32_t(ex->recv.size())) throw invalid("too few recv buffers");
        return ex->punpack->execute(field_ptrs, n_fields, recv_buffers, n_recv, stream);
    });
}

// ---------------------------------------------------------------------------------------------
// zero-copy put (IPC + direct field-to-field copy)
// ---------------------------------------------------------------------------------------------
int ghx_ipc_export(const void* ptr, unsigned char handle[64], uint64_t* offset)
{
    return guarded([&] {
        check_ptr(ptr, "ptr");
        check_ptr(handle, "handle");
        check_ptr(offset, "offset");
        static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, const_cast<void*>(ptr)) != hipSuccess)
            throw hip_error("hipMemGetAddressRange");
        hipIpcMemHandle_t h;
        if (hipIpcGetMemHandle(&h, reinterpret_cast<void*>(base)) != hipSuccess)
        {
            char where[160];
            std::snprintf(where, sizeof(where), "hipIpcGetMemHandle (ptr %p, allocation %p + %zu B)",
                          ptr, reinterpret_cast<void*>(base), size);
            throw hip_error(where);
        }
        std::memcpy(handle, &h, sizeof(h));
        *offset = uint64_t(static_cast<const char*>(ptr) - reinterpret_cast<const char*>(base));
        return GHX_OK;
    });
}

int ghx_ipc_import(const unsigned char handle[64], uint64_t offset, void** base, void** ptr)
{
    return guarded([&] {
        check_ptr(handle, "handle");
        check_ptr(base, "base");
        check_ptr(ptr, "ptr");
        hipIpcMemHandle_t h;
        std::memcpy(&h, handle, sizeof(h));
        void* b = nullptr;
        if (hipIpcOpenMemHandle(&b, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess)
            throw hip_error("hipIpcOpenMemHandle");
        *base = b;
        *ptr = static_cast<char*>(b) + offset;
        return GHX_OK;
    });
}

int ghx_ipc_close(void* base)
{
    return guarded([&] {
        check_ptr(base, "base");
        if (hipIpcCloseMemHandle(base) != hipSuccess) throw hip_error("hipIpcCloseMemHandle");
        return GHX_OK;
    });
}

int ghx_put_create(const ghx_pack_entry* src, int32_t n_src, const ghx_pack_entry* dst,
                   int32_t n_dst, ghx_put** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        if (n_src < 0 || n_dst < 0 || (n_src && !src) || (n_dst && !dst))
            throw invalid("bad entry arrays");
        *out = new ghx_put(src, n_src, dst, n_dst);
        return GHX_OK;
    });
}

int ghx_cs_put_create(const ghx_pack_entry* src, int32_t n_src, const ghx_pack_entry* dst,
                      int32_t n_dst, const ghx_cs_item* dst_cs, const ghx_box* const* dst_global,
                      const int32_t* const* dst_tiles, ghx_put** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        if (n_src < 0 || n_dst < 0 || (n_src && !src) || (n_dst && !dst))
            throw invalid("bad entry arrays");
        if (n_dst && (!dst_cs || !dst_global || !dst_tiles))
            throw invalid("null argument: the target entries' cubed-sphere items, global boxes or tiles");
        *out = new ghx_put(build_cs_put(src, n_src, dst, n_dst, dst_cs, dst_global, dst_tiles));
        return GHX_OK;
    });
}

int ghx_uput_create(const ghx_uput_entry* src, const ghx_uput_entry* dst, int32_t n, ghx_put** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        if (n < 0 || (n && (!src || !dst))) throw invalid("bad entry arrays");
        *out = new ghx_put(std::make_unique<uput_plan>(src, dst, n));
        return GHX_OK;
    });
}

int ghx_uself_create(const ghx_upack_entry* src, const ghx_upack_entry* dst, int32_t n, ghx_uself** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        if (n < 0 || (n && (!src || !dst))) throw invalid("bad entry arrays");
        *out = new ghx_uself{make_uself(src, dst, n)};
        return GHX_OK;
    });
}

int ghx_uself_execute(const ghx_uself* p, void* const* field_ptrs, int32_t n_fields,
                      void* const* buffer_ptrs, int32_t n_buffers, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(p, "plan");
        return p->p->execute_self(field_ptrs, n_fields, buffer_ptrs, n_buffers, stream);
    });
}

int ghx_uself_info(const ghx_uself* p, uint64_t* bytes, int32_t* n_segments, int32_t* n_tiles)
{
    return guarded([&] {
        check_ptr(p, "plan");
        const uplan* peers = p->p->peers.get();  // the mixed form: both parts
        if (bytes) *bytes = p->p->bytes + (peers ? peers->bytes : 0);
        if (n_segments) *n_segments = int32_t(p->p->segs.size()) + (peers ? peers->n_segments : 0);
        if (n_tiles) *n_tiles = int32_t(p->p->recs.size() + p->p->peer_recs.size());
        return GHX_OK;
    });
}

int ghx_umixed_create(const ghx_upack_entry* src, const ghx_upack_entry* dst, int32_t n_self,
                      const ghx_upack_entry* peers, int32_t n_peers, ghx_uself** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        *out = new ghx_uself{make_umixed(src, dst, n_self, peers, n_peers)};
        return GHX_OK;
    });
}

int ghx_umixed_info(const ghx_uself* p, int32_t* n_self_tiles, int32_t* n_peer_segments,
                    int32_t* n_peer_tiles)
{
    return guarded([&] {
        check_ptr(p, "plan");
        if (n_self_tiles) *n_self_tiles = int32_t(p->p->recs.size());
        if (n_peer_segments) *n_peer_segments = p->p->peers ? p->p->peers->n_segments : 0;
        if (n_peer_tiles) *n_peer_tiles = int32_t(p->p->peer_recs.size());
        return GHX_OK;
    });
}

int ghx_umixed_peer_segment(const ghx_uself* p, int32_t k, ghx_usegment_info* out)
{
    return guarded([&] {
        check_ptr(p, "plan");
        check_ptr(out, "out");
        if (!p->p->peers) throw invalid("the plan has no peer part (ghx_uself_create's plan)");
        usegment_info(p->p->peers.get(), k, out);
        return GHX_OK;
    });
}

int ghx_uself_segment(const ghx_uself* p, int32_t k, ghx_uself_segment_info* out)
{
    return guarded([&] {
        check_ptr(p, "plan");
        check_ptr(out, "out");
        const uput_plan& u = *p->p;
        if (k < 0 || size_t(k) >= u.segs.size()) throw invalid("segment index out of range");
        const seg_up& s = u.segs[size_t(k)];
        *out = ghx_uself_segment_info{};
        out->src_field_off = s.src_field_off;
        out->src_index_stride_b = s.src_index_stride_b;
        out->src_level_stride_b = s.src_level_stride_b;
        out->dst_field_off = s.dst_field_off;
        out->dst_index_stride_b = s.dst_index_stride_b;
        out->dst_level_stride_b = s.dst_level_stride_b;
        out->first_index = u.first[size_t(k)];
        out->bytes = s.bytes;
        out->row_bytes = s.row_bytes;
        out->tile_bytes = s.tile_bytes;
        out->n = s.n;
        out->message = u.message[size_t(k)];
        out->n_segments = int32_t(u.segs.size());
        out->src_slot = s.src_slot;
        out->dst_slot = s.dst_slot;
        out->mode = s.mode;
        out->wlog2 = s.wlog2;
        out->src_lid64 = s.src_lid64;
        out->dst_lid64 = s.dst_lid64;
        out->src_runs = s.src_runs;
        out->dst_runs = s.dst_runs;
        out->buf_slot = s.buf_slot;
        out->buf_off = s.buf_off;
        return GHX_OK;
    });
}

int ghx_uself_destroy(ghx_uself* p)
{
    return guarded([&] {
        delete p;
        return GHX_OK;
    });
}

int ghx_uexchange_self_info(const ghx_exchange* ex, int32_t* fusable, int32_t* n_segments,
                            int32_t* n_tiles)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(fusable, "fusable");
        const uput_plan* p = ex->uself.get();
        *fusable = p ? 1 : 0;
        if (n_segments) *n_segments = p ? int32_t(p->segs.size()) : 0;
        if (n_tiles) *n_tiles = p ? int32_t(p->recs.size()) : 0;
        if (!p) set_error(ex->uself_reason);
        return GHX_OK;
    });
}

int ghx_uexchange_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                       void* const* buffers, int32_t n_buffers, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        if (!ex->uself) throw invalid("index-list self exchange: " + ex->uself_reason);
        if (ex->dir_parity[0].word)
            throw invalid("index-list self exchange: the send side has double-buffered buffers "
                          "(ghx_exchange_set_parity); the fused launch writes one copy");
        check_ptr(field_ptrs, "field_ptrs");
        check_ptr(buffers, "buffers");
        return ex->uself->execute_self(field_ptrs, n_fields, buffers, n_buffers, stream);
    });
}

int ghx_uexchange_mixed_info(const ghx_exchange* ex, int32_t* mixed, int32_t* n_self_tiles,
                             int32_t* n_peer_tiles)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(mixed, "mixed");
        const uput_plan* p = ex->umixed.get();
        *mixed = p ? 1 : 0;
        if (n_self_tiles) *n_self_tiles = p ? int32_t(p->recs.size()) : 0;
        if (n_peer_tiles) *n_peer_tiles = p ? int32_t(p->peer_recs.size()) : 0;
        if (!p) set_error(ex->umixed_reason);
        return GHX_OK;
    });
}

namespace
{
// both launches of the index-list mixed form write / read one copy of each buffer
void check_umixed(const ghx_exchange* ex)
{
    check_ptr(ex, "exchange");
    if (!ex->umixed) throw invalid("index-list mixed exchange: " + ex->umixed_reason);
    if (ex->dir_parity[0].word || ex->dir_parity[1].word)
        throw invalid("index-list mixed exchange: the exchange has double-buffered buffers "
                      "(ghx_exchange_set_parity); its launches use one copy");
}
}  // namespace

int ghx_uexchange_pack_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                            void* const* send_buffers, int32_t n_send, ghx_stream stream)
{
    return guarded([&] {
        check_umixed(ex);
        if (n_send < int32_t(ex->send.size())) throw invalid("too few send buffers");
        return ex->umixed->execute_self(field_ptrs, n_fields, send_buffers, n_send, stream);
    });
}

int ghx_uexchange_unpack_peers(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                               void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return guarded([&] {
        check_umixed(ex);
        if (n_recv < int32_t(ex->recv.size())) throw invalid("too few recv buffers");
        if (!ex->upunpack) return int(GHX_OK);  // the rank receives from no peer
        return ex->upunpack->execute(field_ptrs, n_fields, recv_buffers, n_recv, stream);
    });
}

int ghx_uaccum_create(const ghx_upack_entry* contrib, const int32_t* dtypes, int32_t n,
                      const ghx_upack_entry* zero, int32_t n_zero, ghx_uaccum** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        if (n < 0 || n_zero < 0 || (n && (!contrib || !dtypes)) || (n_zero && !zero))
            throw invalid("bad entry arrays");
        *out = new ghx_uaccum(contrib, dtypes, n, zero, n_zero);
        return GHX_OK;
    });
}

int ghx_uaccum_execute(const ghx_uaccum* p, void* const* field_ptrs, int32_t n_fields,
                       void* const* buffer_ptrs, int32_t n_buffers, int32_t zero_halos,
                       ghx_stream stream)
{
    return guarded([&] {
        check_ptr(p, "plan");
        return p->execute(field_ptrs, n_fields, buffer_ptrs, n_buffers, zero_halos != 0, stream);
    });
}

int ghx_uaccum_info(const ghx_uaccum* p, uint64_t* bytes, int64_t* n_dest, int64_t* n_zero_dest,
                    int64_t* n_contrib, int64_t* max_per_dest, int32_t* n_tiles)
{
    return guarded([&] {
        check_ptr(p, "plan");
        if (bytes) *bytes = p->bytes;
        if (n_dest) *n_dest = int64_t(p->n_dest);
        if (n_zero_dest) *n_zero_dest = int64_t(p->n_zero_dest);
        if (n_contrib) *n_contrib = int64_t(p->contribs.size());
        if (max_per_dest) *max_per_dest = p->max_per_dest;
        if (n_tiles) *n_tiles = int32_t(p->tiles.size());
        return GHX_OK;
    });
}

int ghx_uaccum_dest(const ghx_uaccum* p, int64_t k, ghx_uaccum_dest_info* out)
{
    return guarded([&] {
        check_ptr(p, "plan");
        check_ptr(out, "out");
        if (k < 0 || uint64_t(k) >= p->n_dest + p->n_zero_dest) throw invalid("destination index out of range");
        const bool zero = uint64_t(k) >= p->n_dest;
        *out = ghx_uaccum_dest_info{};
        out->field_slot = p->dest_slot[size_t(k)];
        out->zero = zero ? 1 : 0;
        out->lid = p->dest_lid[size_t(k)];
        out->first = zero ? 0 : int64_t(p->ranges[size_t(k)].first);
        out->count = zero ? 0 : int64_t(p->ranges[size_t(k)].count);
        return GHX_OK;
    });
}

int ghx_uaccum_contrib(const ghx_uaccum* p, int64_t j, int32_t* entry, int64_t* pos)
{
    return guarded([&] {
        check_ptr(p, "plan");
        if (j < 0 || uint64_t(j) >= p->contribs.size()) throw invalid("record index out of range");
        if (entry) *entry = int32_t(p->contribs[size_t(j)].entry);
        if (pos) *pos = int64_t(p->contribs[size_t(j)].pos);
        return GHX_OK;
    });
}

int ghx_uaccum_get_create(const ghx_upack_entry* contrib, const int32_t* dtypes, const ghx_upack_entry* const* source,
                          int32_t n, const ghx_upack_entry* zero, int32_t n_zero, ghx_uaccum** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        if (n < 0 || n_zero < 0 || (n && (!contrib || !dtypes)) || (n_zero && !zero)) throw invalid("bad entry arrays");
        check_ptr(source, "source");
        *out = new ghx_uaccum(contrib, dtypes, n, zero, n_zero, source);
        return GHX_OK;
    });
}

int ghx_uaccum_get_execute(const ghx_uaccum* p, void* const* field_ptrs, int32_t n_fields,
                           void* const* buffer_ptrs, int32_t n_buffers, int32_t zero_halos,
                           ghx_stream stream)
{
    return guarded([&] {
        check_ptr(p, "plan");
        return p->execute_get(field_ptrs, n_fields, buffer_ptrs, n_buffers, zero_halos != 0, stream);
    });
}

int ghx_uaccum_contrib_kind(const ghx_uaccum* p, int64_t j, int32_t* kind, int32_t* slot, int64_t* lid)
{
    return guarded([&] {
        check_ptr(p, "plan");
        if (j < 0 || uint64_t(j) >= p->contribs.size()) throw invalid("record index out of range");
        const uint32_t e = p->contribs[size_t(j)].entry;
        const bool field = p->get && p->get_entries[e].field_src;
        if (kind) *kind = field ? 1 : 0;
        if (slot) *slot = field ? int32_t(p->get_entries[e].tab) : int32_t(p->entries[e].buf_slot);
        if (lid) *lid = field ? p->src_lid[size_t(j)] : -1;
        return GHX_OK;
    });
}

int ghx_uaccum_destroy(ghx_uaccum* p)
{
    return guarded([&] {
        delete p;
        return GHX_OK;
    });
}

// The adjoint of an exchange: six kinds of plan set (exchange_plan::adjoint_kind), one create, one
// reverse pack and one accumulate behind the entry points of each.
namespace
{
using adjoint_kind = exchange_plan::adjoint_kind;
using adjoint_set = exchange_plan::adjoint_set;

// per kind: what a launch or a *_plan call says of a set that was not created
const char* const k_no_adjoint[exchange_plan::n_adjoint_kinds] = {
    "adjoint exchange: no adjoint plans (ghx_uexchange_adjoint_create)",
    "adjoint exchange: no adjoint plans (ghx_sexchange_adjoint_create)",
    "fused adjoint exchange: no plans (ghx_sexchange_adjoint_self_create)",
    "cubed-sphere adjoint exchange: no adjoint plans (ghx_cs_exchange_adjoint_create)",
    "fused cubed-sphere adjoint exchange: no plans (ghx_cs_exchange_adjoint_self_create)",
    "fused adjoint exchange: no plans (ghx_uexchange_adjoint_self_create)"};

const adjoint_set* created_adjoint(const ghx_exchange* ex, adjoint_kind kind)
{
    check_ptr(ex, "exchange");
    if (!ex->adjoint[kind].form) throw invalid(k_no_adjoint[kind]);
    return &ex->adjoint[kind];
}

// a launch: both launches of the adjoint use one copy of each buffer
const adjoint_set* check_adjoint(const ghx_exchange* ex, adjoint_kind kind)
{
    const adjoint_set* set = created_adjoint(ex, kind);
    ex->check_single_buffered();
    return set;
}

int adjoint_create(ghx_exchange* ex, adjoint_kind kind, const int32_t* dtypes, int32_t n_items)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        ex->make_adjoint(kind, dtypes, n_items);
        return GHX_OK;
    });
}

int adjoint_pack(const ghx_exchange* ex, adjoint_kind kind, void* const* field_ptrs, int32_t n_fields,
                 void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return guarded([&] {
        const adjoint_set* set = check_adjoint(ex, kind);
        if (n_recv < int32_t(ex->recv.size())) throw invalid("too few recv buffers");
        return set->pack(field_ptrs, n_fields, recv_buffers, n_recv, stream);
    });
}

int adjoint_accumulate(const ghx_exchange* ex, adjoint_kind kind, void* const* field_ptrs, int32_t n_fields,
                       void* const* send_buffers, int32_t n_send, int32_t zero_halos, ghx_stream stream)
{
    return guarded([&] {
        const adjoint_set* set = check_adjoint(ex, kind);
        if (n_send < int32_t(ex->send.size())) throw invalid("too few send buffers");
        return set->accumulate(field_ptrs, n_fields, send_buffers, n_send, zero_halos != 0, stream);
    });
}

// the *_info calls' counts of a structured accumulate plan (null: not created, every count 0)
void saccum_counts(const saccum_plan* p, int64_t* n_boxes, int64_t* n_sources, int64_t* n_field_sources,
                   int64_t* n_rotated_sources)
{
    if (n_boxes) *n_boxes = p ? int64_t(p->n_sum_boxes) : 0;
    if (n_sources) *n_sources = p ? int64_t(p->srcs.size()) : 0;
    if (n_field_sources) *n_field_sources = p ? int64_t(p->n_field_sources) : 0;
    if (n_rotated_sources) *n_rotated_sources = p ? int64_t(p->n_rotated_sources) : 0;
}
}  // namespace

int ghx_uexchange_adjoint_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items)
{
    return adjoint_create(ex, exchange_plan::adj_list, dtypes, n_items);
}

int ghx_uexchange_adjoint_info(const ghx_exchange* ex, int32_t* ready, int64_t* n_dest,
                               int64_t* n_contrib)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(ready, "ready");
        const uaccum_plan* p = ex->adjoint[exchange_plan::adj_list].uaccum.get();
        *ready = p ? 1 : 0;
        if (n_dest) *n_dest = p ? int64_t(p->n_dest) : 0;
        if (n_contrib) *n_contrib = p ? int64_t(p->contribs.size()) : 0;
        return GHX_OK;
    });
}

int ghx_uexchange_adjoint_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                               void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return adjoint_pack(ex, exchange_plan::adj_list, field_ptrs, n_fields, recv_buffers, n_recv, stream);
}

int ghx_uexchange_adjoint_accumulate(const ghx_exchange* ex, void* const* field_ptrs,
                                     int32_t n_fields, void* const* send_buffers, int32_t n_send,
                                     int32_t zero_halos, ghx_stream stream)
{
    return adjoint_accumulate(ex, exchange_plan::adj_list, field_ptrs, n_fields, send_buffers, n_send, zero_halos,
                              stream);
}

int ghx_uexchange_adjoint_self_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items)
{
    return adjoint_create(ex, exchange_plan::adj_list_self, dtypes, n_items);
}

int ghx_uexchange_adjoint_self_info(const ghx_exchange* ex, int32_t* form, int64_t* n_dest, int64_t* n_contrib,
                                    int64_t* n_field_sources)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(form, "form");
        const adjoint_set& set = ex->adjoint[exchange_plan::adj_list_self];
        const uaccum_plan* p = set.uaccum.get();
        *form = set.form;
        if (n_dest) *n_dest = p ? int64_t(p->n_dest) : 0;
        if (n_contrib) *n_contrib = p ? int64_t(p->contribs.size()) : 0;
        if (n_field_sources) *n_field_sources = p ? int64_t(p->n_field_sources) : 0;
        return GHX_OK;
    });
}

int ghx_uexchange_adjoint_self_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                    void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return adjoint_pack(ex, exchange_plan::adj_list_self, field_ptrs, n_fields, recv_buffers, n_recv, stream);
}

int ghx_uexchange_adjoint_self_accumulate(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                          void* const* send_buffers, int32_t n_send, int32_t zero_halos,
                                          ghx_stream stream)
{
    return adjoint_accumulate(ex, exchange_plan::adj_list_self, field_ptrs, n_fields, send_buffers, n_send,
                              zero_halos, stream);
}

int ghx_saccum_create(const ghx_pack_entry* contrib, const int32_t* dtypes, int32_t n,
                      const ghx_pack_entry* zero, int32_t n_zero, ghx_saccum** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        if (n < 0 || n_zero < 0 || (n && (!contrib || !dtypes)) || (n_zero && !zero))
            throw invalid("bad entry arrays");
        *out = new ghx_saccum(contrib, dtypes, n, zero, n_zero);
        return GHX_OK;
    });
}

int ghx_saccum_execute(const ghx_saccum* p, void* const* field_ptrs, int32_t n_fields,
                       void* const* buffer_ptrs, int32_t n_buffers, int32_t zero_halos,
                       ghx_stream stream)
{
    return guarded([&] {
        check_ptr(p, "plan");
        return p->execute(field_ptrs, n_fields, buffer_ptrs, n_buffers, zero_halos != 0, stream);
    });
}

int ghx_saccum_info(const ghx_saccum* p, uint64_t* bytes, int64_t* n_boxes, int64_t* n_zero_boxes,
                    int64_t* n_sources, int64_t* max_sources, int32_t* n_tiles)
{
    return guarded([&] {
        check_ptr(p, "plan");
        if (bytes) *bytes = p->bytes;
        if (n_boxes) *n_boxes = int64_t(p->n_sum_boxes);
        if (n_zero_boxes) *n_zero_boxes = int64_t(p->boxes.size()) - int64_t(p->n_sum_boxes);
        if (n_sources) *n_sources = int64_t(p->srcs.size());
        if (max_sources) *max_sources = p->max_sources;
        if (n_tiles) *n_tiles = int32_t(p->tiles.size());
        return GHX_OK;
    });
}

int ghx_saccum_box(const ghx_saccum* p, int64_t k, ghx_saccum_box_info* out)
{
    return guarded([&] {
        check_ptr(p, "plan");
        check_ptr(out, "out");
        if (k < 0 || uint64_t(k) >= p->boxes.size()) throw invalid("sub-box index out of range");
        const saccum_box& b = p->boxes[size_t(k)];
        *out = ghx_saccum_box_info{};
        out->field_slot = b.field_slot;
        out->zero = b.zero ? 1 : 0;
        for (int d = 0; d < GHX_MAX_DIM; ++d)
        {
            out->first[d] = b.first[d];
            out->last[d] = b.last[d];
        }
        out->row_elems = int64_t(b.row_elems);
        out->wlog2 = b.wlog2;
        out->first_src = b.zero ? 0 : int64_t(b.first_src);
        out->n_src = int64_t(b.n_src);
        return GHX_OK;
    });
}

int ghx_saccum_source(const ghx_saccum* p, int64_t j, int32_t* entry, int32_t* box, int32_t* buffer_slot,
                      uint64_t* buffer_offset_of_origin)
{
    return guarded([&] {
        check_ptr(p, "plan");
        if (j < 0 || uint64_t(j) >= p->srcs.size()) throw invalid("source index out of range");
        if (entry) *entry = int32_t(p->src_entry[size_t(j)]);
        if (box) *box = int32_t(p->src_box[size_t(j)]);
        if (buffer_slot) *buffer_slot = int32_t(p->srcs[size_t(j)].buf_slot);
        if (buffer_offset_of_origin) *buffer_offset_of_origin = p->srcs[size_t(j)].buf_off;
        return GHX_OK;
    });
}

int ghx_saccum_get_create(const ghx_pack_entry* contrib, const int32_t* dtypes, const ghx_pack_entry* const* source,
                          int32_t n, const ghx_pack_entry* zero, int32_t n_zero, ghx_saccum** out)
{
    return guarded([&] {
        check_ptr(out, "out");
        *out = nullptr;
        if (n < 0 || n_zero < 0 || (n && (!contrib || !dtypes)) || (n_zero && !zero)) throw invalid("bad entry arrays");
        check_ptr(source, "source");
        *out = new ghx_saccum(contrib, dtypes, n, zero, n_zero, source);
        return GHX_OK;
    });
}

int ghx_saccum_get_execute(const ghx_saccum* p, void* const* field_ptrs, int32_t n_fields,
                           void* const* buffer_ptrs, int32_t n_buffers, int32_t zero_halos,
                           ghx_stream stream)
{
    return guarded([&] {
        check_ptr(p, "plan");
        return p->execute_get(field_ptrs, n_fields, buffer_ptrs, n_buffers, zero_halos != 0, stream);
    });
}

int ghx_saccum_source_kind(const ghx_saccum* p, int64_t j, int32_t* kind, int32_t* slot, uint64_t* offset_of_origin)
{
    return guarded([&] {
        check_ptr(p, "plan");
        if (j < 0 || uint64_t(j) >= p->srcs.size()) throw invalid("source index out of range");
        const sacc_src& s = p->srcs[size_t(j)];
        if (kind) *kind = (s.flags & kSaccFieldSrc) ? 1 : 0;
        if (slot) *slot = p->get ? p->tab_slot[s.buf_slot] : int32_t(s.buf_slot);
        if (offset_of_origin) *offset_of_origin = s.buf_off;
        return GHX_OK;
    });
}

int ghx_saccum_destroy(ghx_saccum* p)
{
    return guarded([&] {
        delete p;
        return GHX_OK;
    });
}

int ghx_sexchange_adjoint_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items)
{
    return adjoint_create(ex, exchange_plan::adj_boxes, dtypes, n_items);
}

int ghx_sexchange_adjoint_info(const ghx_exchange* ex, int32_t* ready, int64_t* n_boxes, int64_t* n_sources)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(ready, "ready");
        const adjoint_set& set = ex->adjoint[exchange_plan::adj_boxes];
        *ready = set.form ? 1 : 0;
        saccum_counts(set.saccum.get(), n_boxes, n_sources, nullptr, nullptr);
        return GHX_OK;
    });
}

int ghx_sexchange_adjoint_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                               void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return adjoint_pack(ex, exchange_plan::adj_boxes, field_ptrs, n_fields, recv_buffers, n_recv, stream);
}

int ghx_sexchange_adjoint_accumulate(const ghx_exchange* ex, void* const* field_ptrs,
                                     int32_t n_fields, void* const* send_buffers, int32_t n_send,
                                     int32_t zero_halos, ghx_stream stream)
{
    return adjoint_accumulate(ex, exchange_plan::adj_boxes, field_ptrs, n_fields, send_buffers, n_send, zero_halos,
                              stream);
}

int ghx_sexchange_adjoint_self_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items)
{
    return adjoint_create(ex, exchange_plan::adj_boxes_self, dtypes, n_items);
}

int ghx_sexchange_adjoint_self_info(const ghx_exchange* ex, int32_t* form, int64_t* n_boxes, int64_t* n_sources,
                                    int64_t* n_field_sources)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(form, "form");
        const adjoint_set& set = ex->adjoint[exchange_plan::adj_boxes_self];
        *form = set.form;
        saccum_counts(set.saccum.get(), n_boxes, n_sources, n_field_sources, nullptr);
        return GHX_OK;
    });
}

int ghx_sexchange_adjoint_self_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                    void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return adjoint_pack(ex, exchange_plan::adj_boxes_self, field_ptrs, n_fields, recv_buffers, n_recv, stream);
}

int ghx_sexchange_adjoint_self_accumulate(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                          void* const* send_buffers, int32_t n_send, int32_t zero_halos,
                                          ghx_stream stream)
{
    return adjoint_accumulate(ex, exchange_plan::adj_boxes_self, field_ptrs, n_fields, send_buffers, n_send,
                              zero_halos, stream);
}

int ghx_cs_exchange_adjoint_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items)
{
    return adjoint_create(ex, exchange_plan::adj_cs, dtypes, n_items);
}

int ghx_cs_exchange_adjoint_info(const ghx_exchange* ex, int32_t* ready, int64_t* n_boxes, int64_t* n_sources,
                                 int32_t* n_pack_x_records, int32_t* n_pack_x_tiles)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(ready, "ready");
        const adjoint_set& set = ex->adjoint[exchange_plan::adj_cs];
        *ready = set.form ? 1 : 0;
        saccum_counts(set.saccum.get(), n_boxes, n_sources, nullptr, nullptr);
        if (n_pack_x_records) *n_pack_x_records = set.xpack ? set.xpack->n_records : 0;
        if (n_pack_x_tiles) *n_pack_x_tiles = set.xpack ? int32_t(set.xpack->n_tiles) : 0;
        return GHX_OK;
    });
}

int ghx_cs_exchange_adjoint_plan(const ghx_exchange* ex, const ghx_saccum** out)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(out, "out");
        *out = created_adjoint(ex, exchange_plan::adj_cs)->saccum.get();
        return GHX_OK;
    });
}

int ghx_cs_exchange_adjoint_segments(const ghx_exchange* ex, int32_t* n_pack_segments, int32_t* n_unpack_segments)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        const adjoint_set& set = ex->adjoint[exchange_plan::adj_cs];
        if (n_pack_segments) *n_pack_segments = set.spack ? set.spack->n_segments : 0;
        if (n_unpack_segments) *n_unpack_segments = ex->cubed_sphere && ex->sunpack ? ex->sunpack->n_segments : 0;
        return GHX_OK;
    });
}

int ghx_cs_exchange_adjoint_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                 void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return adjoint_pack(ex, exchange_plan::adj_cs, field_ptrs, n_fields, recv_buffers, n_recv, stream);
}

int ghx_cs_exchange_adjoint_accumulate(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                       void* const* send_buffers, int32_t n_send, int32_t zero_halos,
                                       ghx_stream stream)
{
    return adjoint_accumulate(ex, exchange_plan::adj_cs, field_ptrs, n_fields, send_buffers, n_send, zero_halos,
                              stream);
}

int ghx_cs_exchange_adjoint_self_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items)
{
    return adjoint_create(ex, exchange_plan::adj_cs_self, dtypes, n_items);
}

int ghx_cs_exchange_adjoint_self_info(const ghx_exchange* ex, int32_t* form, int64_t* n_boxes, int64_t* n_sources,
                                      int64_t* n_field_sources, int64_t* n_rotated_sources)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(form, "form");
        const adjoint_set& set = ex->adjoint[exchange_plan::adj_cs_self];
        *form = set.form;
        saccum_counts(set.saccum.get(), n_boxes, n_sources, n_field_sources, n_rotated_sources);
        return GHX_OK;
    });
}

int ghx_cs_exchange_adjoint_self_plan(const ghx_exchange* ex, const ghx_saccum** out)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        check_ptr(out, "out");
        *out = created_adjoint(ex, exchange_plan::adj_cs_self)->saccum.get();
        return GHX_OK;
    });
}

int ghx_cs_exchange_adjoint_self_segments(const ghx_exchange* ex, int32_t* n_pack_segments, int32_t* n_pack_x_records)
{
    return guarded([&] {
        check_ptr(ex, "exchange");
        const adjoint_set& set = ex->adjoint[exchange_plan::adj_cs_self];
        if (n_pack_segments) *n_pack_segments = set.spack ? set.spack->n_segments : 0;
        if (n_pack_x_records) *n_pack_x_records = set.xpack ? set.xpack->n_records : 0;
        return GHX_OK;
    });
}

int ghx_saccum_source_map(const ghx_saccum* p, int64_t j, int64_t* strides, int32_t* neg_mask, int32_t* comp_dim)
{
    return guarded([&] {
        check_ptr(p, "plan");
        if (j < 0 || uint64_t(j) >= p->srcs.size()) throw invalid("source index out of range");
        const saccum_plan::source_map& m = p->src_map[size_t(j)];
        for (int d = 0; strides && d < GHX_MAX_DIM; ++d) strides[d] = m.stride[d];
        if (neg_mask) *neg_mask = m.neg;
        if (comp_dim) *comp_dim = m.comp_dim;
        return GHX_OK;
    });
}

int ghx_cs_exchange_adjoint_self_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                      void* const* recv_buffers, int32_t n_recv, ghx_stream stream)
{
    return adjoint_pack(ex, exchange_plan::adj_cs_self, field_ptrs, n_fields, recv_buffers, n_recv, stream);
}

int ghx_cs_exchange_adjoint_self_accumulate(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                            void* const* send_buffers, int32_t n_send, int32_t zero_halos,
                                            ghx_stream stream)
{
    return adjoint_accumulate(ex, exchange_plan::adj_cs_self, field_ptrs, n_fields, send_buffers, n_send, zero_halos,
                              stream);
}

int ghx_uput_segment(const ghx_put* put, int32_t k, ghx_uput_segment_info* out)
{
    return guarded([&] {
        check_ptr(put, "put");
        check_ptr(out, "out");
        const uput_plan* p = put->u.get();
        if (!p) throw invalid("not a put of ghx_uput_create");
        if (k < 0 || size_t(k) >= p->segs.size()) throw invalid("segment index out of range");
        const seg_up& s = p->segs[size_t(k)];
        *out = ghx_uput_segment_info{};
        out->src_field_off = s.src_field_off;
        out->src_index_stride_b = s.src_index_stride_b;
        out->src_level_stride_b = s.src_level_stride_b;
        out->dst_field_off = s.dst_field_off;
        out->dst_index_stride_b = s.dst_index_stride_b;
        out->dst_level_stride_b = s.dst_level_stride_b;
        out->first_index = p->first[size_t(k)];
        out->bytes = s.bytes;
        out->row_bytes = s.row_bytes;
        out->tile_bytes = s.tile_bytes;
        out->n = s.n;
        out->message = p->message[size_t(k)];
        out->n_segments = int32_t(p->segs.size());
        out->src_slot = s.src_slot;
        out->dst_slot = s.dst_slot;
        out->mode = s.mode;
        out->wlog2 = s.wlog2;
        out->src_lid64 = s.src_lid64;
        out->dst_lid64 = s.dst_lid64;
        out->src_runs = s.src_runs;
        out->dst_runs = s.dst_runs;
        return GHX_OK;
    });
}

int ghx_cs_put_info(const ghx_put* put, int32_t* n_pair_tiles, int32_t* n_x_records,
                    int32_t* n_x_tiles)
{
    return guarded([&] {
        check_ptr(put, "put");
        const cs_put_plan* p = put->cs.get();
        if (put->u)
        {
            if (n_pair_tiles) *n_pair_tiles = int32_t(put->u->recs.size());
            if (n_x_records) *n_x_records = 0;
            if (n_x_tiles) *n_x_tiles = 0;
            return GHX_OK;
        }
        if (n_pair_tiles) *n_pair_tiles = p ? int32_t(p->n_pair_tiles()) : int32_t(put->from->first().n_tiles);
        if (n_x_records) *n_x_records = p ? p->n_x_records : 0;
        if (n_x_tiles) *n_x_tiles = p ? int32_t(p->n_x_tiles()) : 0;
        return GHX_OK;
    });
}

int ghx_put_execute(const ghx_put* put, void* const* src_fields, int32_t n_src,
                    void* const* dst_fields, int32_t n_dst, ghx_stream stream)
{
    return guarded([&] {
        check_ptr(put, "put");
        if (put->cs || put->u)
        {
            check_ptr(src_fields, "src_fields");
            check_ptr(dst_fields, "dst_fields");
        }
        return put->execute(src_fields, n_src, dst_fields, n_dst, stream);
    });
}

int ghx_put_info(const ghx_put* put, uint64_t* bytes, int32_t* n_tiles)
{
    return guarded([&] {
        check_ptr(put, "put");
        if (put->cs)
        {
            if (bytes) *bytes = put->cs->bytes;
            if (n_tiles) *n_tiles = int32_t(put->cs->n_pair_tiles() + put->cs->n_x_tiles());
            return GHX_OK;
        }
        if (put->u)
        {
            if (bytes) *bytes = put->u->bytes;
            if (n_tiles) *n_tiles = int32_t(put->u->recs.size());
            return GHX_OK;
        }
        if (bytes) *bytes = put->from->bytes;
        if (n_tiles) *n_tiles = int32_t(put->from->first().n_tiles);
        return GHX_OK;
    });
}

int ghx_put_destroy(ghx_put* put)
{
    return guarded([&] {
        delete put;
        return GHX_OK;
    });
}

}  // extern "C"
