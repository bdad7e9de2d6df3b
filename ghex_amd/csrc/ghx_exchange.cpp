// ghx_exchange.cpp — the exchange planner (communication_object::allocate semantics: buffers per
// domain pair, fields in item order), the fused self / mixed / cubed-sphere plans built with an
// exchange, the put plans, and the paired launch (k_self, k_put) they execute.
#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "ghx_cubed_sphere.hpp"
#include "ghx_exchange.hpp"
#include "ghx_pattern.hpp"
#include "ghx_plan.hpp"

namespace ghx
{
namespace
{
// One paired launch (`launch`: launch_self or launch_put), tiled by the primary group `p` alone:
// `companion` is the device table of the segments paired with p's, `pair_recs` the pair records
// of the two (null: the tile table path). The first `n_first` pointers of `first` fill the
// field slots and the first `n_second` of `second` the buffer slots (a put's target fields);
// the names are those of the null refusals. `parity`: double-buffered buffers, if any.
int launch_paired(int (*launch)(const kargs&, void*, uint32_t), const launch_group<seg_s>& p,
                  const void* companion, const void* pair_recs, void* const* first, int n_first,
                  const char* first_name, void* const* second, int n_second,
                  const char* second_name, const parity_cfg* parity, void* stream)
{
    if (!p.dev.segs || !companion) throw hip_error("plan has no device tables");
    kargs a{};
    a.segs = p.dev.segs;
    a.segs2 = companion;
    a.tile_seg = p.dev.tiles;
    a.tile_recs = pair_recs;
    a.n_tiles = p.n_tiles;
    fill_slots(a.field_ptr, first, {}, n_first, first_name);
    fill_slots(a.buf_ptr, second, {}, n_second, second_name);
    if (parity) parity->apply(a, {}, n_second);
    return launch(a, stream, grid_for_tiles(p.n_tiles));
}

// Every recv buffer aliases the send buffer of the same pair, and pack segment k and unpack
// segment k cover the same buffer bytes: pack and unpack may be fused (exchange_plan::self_ok)
bool all_self(const exchange_plan& ex)
{
    bool ok = ex.cs_rotated == 0 && !ex.upack && !ex.uunpack && ex.spack && ex.sunpack &&
              ex.send.size() == ex.recv.size() && !ex.spack->grouped() && !ex.sunpack->grouped();
    for (size_t i = 0; ok && i < ex.send.size(); ++i)
        ok = ex.send[i].first_id == ex.recv[i].first_id && ex.send[i].second_id == ex.recv[i].second_id &&
             ex.send[i].size == ex.recv[i].size;
    return ok && exchange_plan::same_messages(*ex.spack, *ex.sunpack);
}

// The sending spaces of build_cs_self and build_cs_put by where their message bytes start:
// (buffer slot, byte offset) -> the entry and its box
struct space
{
    const ghx_pack_entry* e;
    const ghx_box* box;
};
using space_index = std::map<std::pair<int32_t, uint64_t>, space>;
// false: another space was there (and is replaced)
bool add_space(space_index& idx, const ghx_pack_entry& e, const ghx_box& box, uint64_t off)
{
    return idx.insert_or_assign({e.buffer_slot, off}, space{&e, &box}).second;
}
uint64_t box_bytes(const ghx_pack_entry& e, const ghx_box& b)
{
    uint64_t n = uint64_t(e.field.num_components) * uint64_t(e.field.elem_size);
    for (int d = 0; d < 3; ++d) n *= uint64_t(int64_t(b.last[d]) - b.first[d] + 1);
    return n;
}

// communication_object::allocate (include/ghex/communication_object.hpp:1019-1066)
void plan_direction(const ghx_exchange_item* items, int n_items, bool receive,
                    std::vector<xbuffer>& bufs_out, std::vector<ghx_pack_entry>& sent,
                    std::vector<ghx_upack_entry>& uent, std::vector<std::vector<ghx_box>>& box_store,
                    std::vector<const halo_entry*>* sent_halos = nullptr)
{
    struct finfo
    {
        int item;
        const halo_entry* e;
        uint64_t offset;
    };
    struct buf
    {
        xbuffer x;
        std::vector<finfo> fields;
    };
    std::map<std::pair<int32_t, int32_t>, buf> mem;  // domain_id_pair ordering (:165-174)
    for (int k = 0; k < n_items; ++k)
    {
        const auto& it = items[k];
        if (!it.pattern) throw invalid("exchange item without pattern");
        const auto& ps = *it.pattern;
        if (it.local_index < 0 || it.local_index >= int(ps.doms.size()))
            throw invalid("exchange item local_index out of range");
        if ((it.kind == 0) != (ps.kind == 0)) throw invalid("field kind does not match pattern kind");
        if (it.align < 1 || (it.align & (it.align - 1))) throw invalid("align must be a power of two");
        const auto& dp = ps.doms[size_t(it.local_index)];
        const auto& halos = receive ? dp.recv : dp.send;
        int64_t nc, elem;
        if (it.kind == 0)
        {
            validate_field(it.field);
            nc = it.field.num_components;
            elem = it.field.elem_size;
        }
        else
        {
            nc = it.udata.levels;
            elem = it.udata.elem_size;
        }
        for (const auto& e : halos)
        {
            int64_t n = 0;
            if (it.kind == 0)
                for (const auto& b : e.boxes) n += b.size(ps.dim);
            else n = int64_t(e.lids.size());
            n *= nc;
            if (n < 1) continue;
            const auto pair = receive ? std::make_pair(dp.id, e.key.remote_id)
                                      : std::make_pair(e.key.remote_id, dp.id);
            auto bi = mem.find(pair);
            if (bi == mem.end())
            {
                buf b;
                b.x = {pair.first, pair.second, e.key.remote_rank, e.key.tag + it.tag_offset, 0};
                bi = mem.emplace(pair, std::move(b)).first;
            }
            const uint64_t prev = bi->second.x.size;
            const uint64_t a = uint64_t(it.align);
            const uint64_t pad = ((prev + a - 1) / a) * a - prev;
            bi->second.fields.push_back({k, &e, prev + pad});
            bi->second.x.size += pad + uint64_t(n) * uint64_t(elem);
        }
    }
    int32_t slot = 0;
    for (auto& kv : mem)
    {
        bufs_out.push_back(kv.second.x);
        for (const auto& fi : kv.second.fields)
        {
            const auto& it = items[fi.item];
            if (it.kind == 0)
            {
                const int dim = it.pattern->dim;
                box_store.emplace_back();
                auto& bx = box_store.back();
                for (const auto& b : fi.e->boxes)
                {
                    ghx_box g{};
                    for (int d = 0; d < dim; ++d)
                    {
                        g.first[d] = b.lf[d];
                        g.last[d] = b.ll[d];
                    }
                    bx.push_back(g);
                }
                if (it.field.dim - (it.field.has_components ? 1 : 0) != dim)
                    throw invalid("field spatial dimension does not match the pattern");
                ghx_pack_entry pe{};
                pe.field = it.field;
                pe.field_slot = fi.item;
                pe.buffer_slot = slot;
                pe.buffer_offset = fi.offset;
                pe.boxes = bx.data();
                pe.n_boxes = int32_t(bx.size());
                sent.push_back(pe);
                if (sent_halos) sent_halos->push_back(fi.e);
            }
            else
            {
                ghx_upack_entry ue{};
                ue.data = it.udata;
                ue.field_slot = fi.item;
                ue.buffer_slot = slot;
                ue.buffer_offset = fi.offset;
                ue.lids = fi.e->lids.data();
                ue.n_lids = int64_t(fi.e->lids.size());
                uent.push_back(ue);
            }
        }
        ++slot;
    }
}

// Exchanges with self AND peer messages — a rank whose periodic wrap reaches itself next to real
// neighbours, e.g. the (2,1,1) and (2,2,1) decompositions: the pack launch also writes the halos
// of the self messages straight from the registers it packs them from (k_self's forwarding path),
// and the unpack launch covers the peer messages only. Companion segment k of the pack plan is
// the unpack segment of the same buffer bytes for a self message (same tiling, checked), or
// zero for a peer message. `rent` = the receive-side pack entries of every recv buffer.
// per recv buffer of rank `me` the send buffer of the same pair of domains, size and rank: a self
// message, whose recv buffer IS its send buffer; -1 for a peer's
std::vector<int> self_pairs(const exchange_plan& ex, int32_t me)
{
    std::vector<int> send_of_recv(ex.recv.size(), -1);
    for (size_t j = 0; j < ex.recv.size(); ++j)
    {
        const xbuffer& r = ex.recv[j];
        if (r.rank != me) continue;
        for (size_t i = 0; i < ex.send.size(); ++i)
        {
            const xbuffer& s = ex.send[i];
            if (s.rank == me && s.first_id == r.first_id && s.second_id == r.second_id &&
                s.size == r.size)
            {
                send_of_recv[j] = int(i);
                break;
            }
        }
    }
    return send_of_recv;
}

void build_mixed(exchange_plan& ex, int32_t me, const std::vector<ghx_pack_entry>& rent)
{
    if (!ex.spack || !ex.sunpack || ex.upack || ex.uunpack || me < 0 || ex.self_fusable()) return;
    const std::vector<int> send_of_recv = self_pairs(ex, me);
    const bool any_self = std::any_of(send_of_recv.begin(), send_of_recv.end(), [](int i) { return i >= 0; });
    if (!any_self) return;
    std::vector<ghx_pack_entry> self_e, peer_e;
    for (const ghx_pack_entry& e : rent)
    {
        const int i = send_of_recv[size_t(e.buffer_slot)];
        if (i < 0)
        {
            peer_e.push_back(e);
            continue;
        }
        ghx_pack_entry s = e;
        s.buffer_slot = i;  // a self message's recv buffer IS its send buffer
        self_e.push_back(s);
    }
    if (peer_e.empty()) return;
    std::stable_sort(self_e.begin(), self_e.end(),
                     [](const ghx_pack_entry& a, const ghx_pack_entry& b) {
                         return a.buffer_slot < b.buffer_slot;
                     });
    if (ex.spack->grouped()) return;  // more slots than one launch holds: two-launch path
    const splan su(self_e.data(), int(self_e.size()), 1);
    if (su.grouped()) return;
    std::vector<char> is_self(ex.send.size(), 0);
    for (int i : send_of_recv)
        if (i >= 0) is_self[size_t(i)] = 1;
    const std::vector<seg_s>& ps = ex.spack->first().host_segs;
    const std::vector<seg_s>& us = su.first().host_segs;
    std::vector<seg_s> comp(ps.size());  // value-initialised: bytes = 0 -> pack only
    size_t m = 0;
    bool short_self = false;
    for (size_t k = 0; k < ps.size(); ++k)
    {
        if (!is_self[ps[k].buf_slot]) continue;
        short_self = short_self || ps[k].row_bytes < g_tune.small_row_bytes;
        if (m >= us.size()) return;
        const seg_s& q = us[m++];
        if (!exchange_plan::same_message(ps[k], q) || q.bytes == 0) return;
        comp[k] = q;
    }
    if (m != us.size()) return;
    // Worth it only when the self messages include request-bound short rows (the unit-stride
    // x-faces of an x-local decomposition such as (1,1,2)): fusing their reads and writes into
    // one launch is what the fused self exchange gains. Self messages of long rows alone (the
    // y/z wrap of a (2,1,1) decomposition) measured 1-3 % slower mixed than plain
    // (tools/emu_rank_bench.py, profiles/r01c_emu_rank.jsonl).
    if (!short_self && !g_tune.mixed_always) return;
    upload_segments(ex.mixed_comp, comp);
    upload_pair_records(ex.mixed_recs, ps, comp, ex.spack->first().host_tiles);
    ex.mixed_max_field_slot = su.max_field_slot;
    ex.punpack = std::make_unique<splan>(peer_e.data(), int(peer_e.size()), 1);
    ex.mixed = true;
}

// One receive (target) space against the send (source) space at the same message bytes, for
// build_cs_self and build_cs_put. A space that cs_plan_space plans as ordinary segments which the
// sender's add_box_segments match one to one pairs: `from` / `to` hold segment k of each side over
// the same bytes, slots unset. Every other space becomes `box`: the receiving side's dense box
// (field slot re.field_slot, buffer slot `buf_slot`) with the sending side of the same cells.
// Throws `invalid` with the reason for what neither form can serve.
struct cs_pairing
{
    bool paired = false;
    std::vector<seg_s> from, to;
    xsbox box{};
    uint64_t bytes = 0;  // the space's message bytes
};
cs_pairing pair_cs_space(const ghx_pack_entry& se, const ghx_box& sbox, const ghx_pack_entry& re,
                         const ghx_cs_item& item, const is_pair& space, int32_t tile,
                         int32_t buf_slot, uint64_t off)
{
    const ghx_field_desc& fs = se.field;
    const ghx_field_desc& fr = re.field;
    bool same = fs.elem_size == fr.elem_size && fs.dim == fr.dim &&
                fs.has_components == fr.has_components && fs.num_components == fr.num_components;
    for (int d = 0; same && d < fr.dim; ++d) same = fs.layout[d] == fr.layout[d];
    if (!same)
        throw invalid("the two fields of a message differ in element size, components or "
                      "layout order (the message's axis order differs between the two sides)");
    cs_pairing pr;
    cs_recv_plan rp;
    cs_plan_space(rp, fr, item, space, tile, re.field_slot, re.buffer_slot, off, &pr.bytes);
    add_box_segments(pr.from, fs, sbox, 0, 0, off);  // also checks the source's bounds
    pr.paired = rp.xs.empty() && pr.from.size() == rp.segs.size();
    for (size_t i = 0; pr.paired && i < pr.from.size(); ++i)
        pr.paired = exchange_plan::same_message(pr.from[i], rp.segs[i]);
    if (pr.paired)
    {
        pr.to = rp.segs;
        return pr;
    }
    pr.from.clear();
    const int64_t elem = fr.elem_size;
    if (elem > 16 || (elem & (elem - 1)))
        throw invalid("a space that cannot be paired holds elements that are not 1, 2, 4, 8 or 16 bytes");
    xsbox& x = pr.box;
    x.dst = rp.xs.empty() ? cs_space_box(fr, item, space, tile, re.field_slot, buf_slot, off) : rp.xs[0];
    // the sending side of the same dense box: its axes are the sender's dims in layout order,
    // fastest first — the receiver's order, the layouts being equal
    const int D = fs.dim;
    int by_speed[GHX_MAX_DIM];
    for (int d = 0; d < D; ++d) by_speed[D - 1 - fs.layout[d]] = d;
    x.src_off = 0;
    for (int d = 0; d < 3; ++d) x.src_off += (int64_t(sbox.first[d]) + fs.offsets[d]) * fs.byte_strides[d];
    for (int a = 0; a < 4; ++a) x.src_stride[a] = 0;
    for (int a = 0; a < D; ++a)
    {
        const int d = by_speed[a];
        const int64_t ext = d < 3 ? int64_t(sbox.last[d]) - sbox.first[d] + 1 : int64_t(fs.num_components);
        if (ext != int64_t(x.dst.ext[a]))
            throw invalid("a source box and its target box differ in shape under the tile transform");
        x.src_stride[a] = fs.byte_strides[d];
    }
    x.src_slot = se.field_slot;
    return pr;
}

// The fused self exchange of a cubed-sphere exchange (cs_self_plan, k_self_cs), built device-less
// with the exchange; left absent, with the reason in ex.cs_self_reason, when the exchange has a
// message that leaves the rank, has more pointers than the launch's table, pairs fields of different
// element size or layout order, or reads a cell it writes. `rhalos`: the halo entry behind each
// of ex.entries[1].
void build_cs_self(exchange_plan& ex, const ghx_cs_item* cs, int32_t me,
                   const std::vector<const halo_entry*>& rhalos)
{
    const std::vector<ghx_pack_entry>& sent = ex.entries[0];
    const std::vector<ghx_pack_entry>& rent = ex.entries[1];
    auto refuse = [&](const char* why) {
        ex.cs_self.reset();
        ex.cs_self_reason = std::string("not fusable: ") + why;
    };
    bool self = ex.send.size() == ex.recv.size() && !ex.send.empty();
    for (size_t i = 0; self && i < ex.send.size(); ++i)
        self = ex.send[i].first_id == ex.recv[i].first_id && ex.send[i].second_id == ex.recv[i].second_id &&
               ex.send[i].size == ex.recv[i].size && ex.send[i].rank == me && ex.recv[i].rank == me;
    if (!self) return refuse("the exchange has peer messages (a recv buffer that is not the send buffer of the same domain pair on this rank)");
    if (!ex.uentries[0].empty() || !ex.uentries[1].empty() || ex.upack || ex.uunpack)
        return refuse("the exchange has unstructured items");
    if (size_t(ex.n_items) + ex.send.size() > size_t(kCsSelfPtrs) || !ex.spack)
        return refuse("more field and buffer slots than one fused launch's arguments hold (it would need several launch groups)");
    space_index by_bytes;  // the send spaces by the buffer bytes they occupy
    for (const ghx_pack_entry& e : sent)
    {
        uint64_t off = e.buffer_offset;
        for (int b = 0; b < e.n_boxes; ++b)
        {
            add_space(by_bytes, e, e.boxes[b], off);
            off += box_bytes(e, e.boxes[b]);
        }
    }
    // Source check: every source box lies in its field's own domain cells — at or above local
    // cell 0 in x and y, and clear of every box the exchange writes into that field (the domain's
    // upper corner is not part of a cubed-sphere item; the receive boxes are what must be missed).
    // No cell the launch reads is then a cell it writes.
    for (const ghx_pack_entry& e : sent)
        for (int b = 0; b < e.n_boxes; ++b)
        {
            const ghx_box& s = e.boxes[b];
            if (s.first[0] < 0 || s.first[1] < 0 || s.first[2] < 0)
                return refuse("a source box reaches into its field's halo");
            for (size_t k = 0; k < rent.size(); ++k)
            {
                if (rent[k].field_slot != e.field_slot) continue;
                for (const is_pair& w : rhalos[k]->boxes)
                {
                    bool meet = true;
                    for (int d = 0; d < 3; ++d) meet = meet && s.first[d] <= w.ll[d] && w.lf[d] <= s.last[d];
                    if (meet) return refuse("a source box reaches into its field's halo (cells the exchange writes)");
                }
            }
        }
    std::vector<seg_s> pack, unpack;
    std::vector<int32_t> gf_p, gf_u, gb;
    std::vector<xsbox> boxes;
    for (size_t k = 0; k < rent.size(); ++k)
    {
        const ghx_pack_entry& re = rent[k];
        const halo_entry& he = *rhalos[k];
        uint64_t off = re.buffer_offset;
        for (size_t b = 0; b < he.boxes.size(); ++b)
        {
            const auto it = by_bytes.find({re.buffer_slot, off});
            if (it == by_bytes.end())
                return refuse("a receive space has no send space at the same buffer bytes");
            cs_pairing pr;
            try
            {
                pr = pair_cs_space(*it->second.e, *it->second.box, re, cs[re.field_slot], he.boxes[b],
                                   he.tiles[b], re.buffer_slot, off);
            }
            catch (const invalid& e)
            {
                return refuse(e.what());
            }
            for (size_t i = 0; i < pr.from.size(); ++i)
            {
                pack.push_back(pr.from[i]);
                unpack.push_back(pr.to[i]);
                gf_p.push_back(it->second.e->field_slot);
                gf_u.push_back(re.field_slot);
                gb.push_back(re.buffer_slot);
            }
            if (!pr.paired) boxes.push_back(pr.box);
            off += pr.bytes;
        }
    }
    try
    {
        ex.cs_self = std::make_unique<cs_self_plan>(pack, unpack, gf_p, gf_u, gb, boxes);
        ex.cs_self_reason.clear();
    }
    catch (const invalid& e)
    {
        refuse(e.what());
    }
}

// The fused self exchange of an exchange of unstructured items (uput_plan with its buffer side,
// k_self_u), built device-less with the exchange; left absent, with the reason in
// ex.uself_reason, when the exchange has a structured item, no message, a message that leaves
// the rank, or what make_uself refuses. A message's unpack entry is the one at its pack entry's
// (buffer slot, buffer offset): recv buffer i is send buffer i.
void build_uself(exchange_plan& ex, int32_t me)
{
    const std::vector<ghx_upack_entry>& sent = ex.uentries[0];
    const std::vector<ghx_upack_entry>& rent = ex.uentries[1];
    auto refuse = [&](const std::string& why) {
        ex.uself.reset();
        ex.uself_reason = "not fusable: " + why;
    };
    if (ex.spack || ex.sunpack || !ex.entries[0].empty() || !ex.entries[1].empty())
        return refuse("the exchange has structured items");
    if (sent.empty() && rent.empty()) return refuse("the exchange has no message");
    bool self = ex.send.size() == ex.recv.size();
    for (size_t i = 0; self && i < ex.send.size(); ++i)
        self = ex.send[i].first_id == ex.recv[i].first_id && ex.send[i].second_id == ex.recv[i].second_id &&
               ex.send[i].size == ex.recv[i].size && ex.send[i].rank == me && ex.recv[i].rank == me;
    if (!self) return refuse("the exchange has peer messages (a recv buffer that is not the send buffer of the same domain pair on this rank)");
    std::map<std::pair<int32_t, uint64_t>, const ghx_upack_entry*> by_bytes;
    for (const ghx_upack_entry& e : sent) by_bytes[{e.buffer_slot, e.buffer_offset}] = &e;
    if (by_bytes.size() != sent.size() || sent.size() != rent.size())
        return refuse("the pack and unpack entries do not pair one to one");
    std::vector<ghx_upack_entry> src, dst;
    for (const ghx_upack_entry& r : rent)
    {
        const auto it = by_bytes.find({r.buffer_slot, r.buffer_offset});
        if (it == by_bytes.end()) return refuse("an unpack entry has no pack entry at the same buffer bytes");
        src.push_back(*it->second);
        dst.push_back(r);
    }
    try
    {
        ex.uself = make_uself(src.data(), dst.data(), int(src.size()));
        ex.uself_reason.clear();
    }
    catch (const invalid& e)
    {
        refuse(e.what());
    }
}

// The mixed form of an exchange of unstructured items with self AND peer messages (make_umixed,
// k_pack_self_u), built device-less with the exchange: the pack launch also stores the self
// messages' halos, the unpack launch (ex.upunpack) covers the peer recv buffers only. A recv
// buffer is a self message when it belongs to this rank and a send buffer of the same domain
// pair, size and rank exists (build_mixed's match); its unpack entries pair with the pack entries
// at the same (send buffer slot, buffer offset). Left absent, with the reason in
// ex.umixed_reason, when the exchange has a structured item, no self or no peer message, entries
// that do not pair, or what make_umixed refuses.
void build_umixed(exchange_plan& ex, int32_t me)
{
    const std::vector<ghx_upack_entry>& sent = ex.uentries[0];
    const std::vector<ghx_upack_entry>& rent = ex.uentries[1];
    auto refuse = [&](const std::string& why) {
        ex.umixed.reset();
        ex.upunpack.reset();
        ex.umixed_reason = "not mixed: " + why;
    };
    if (ex.spack || ex.sunpack || !ex.entries[0].empty() || !ex.entries[1].empty())
        return refuse("the exchange has structured items");
    std::vector<int> send_of_recv(ex.recv.size(), -1);
    std::vector<char> self_send(ex.send.size(), 0);
    bool any_self = false, any_peer = false;
    for (size_t j = 0; j < ex.recv.size(); ++j)
    {
        const xbuffer& r = ex.recv[j];
        any_peer = any_peer || r.rank != me;
        if (r.rank != me) continue;
        for (size_t i = 0; i < ex.send.size(); ++i)
        {
            const xbuffer& s = ex.send[i];
            if (s.rank == me && !self_send[i] && s.first_id == r.first_id && s.second_id == r.second_id &&
                s.size == r.size)
            {
                send_of_recv[j] = int(i);
                self_send[i] = 1;
                any_self = true;
                break;
            }
        }
    }
    for (const xbuffer& s : ex.send) any_peer = any_peer || s.rank != me;
    if (!any_self)
        return refuse("the exchange has no self message (no recv buffer that is the send buffer of "
                      "the same domain pair on this rank)");
    if (!any_peer) return refuse("the exchange has no peer message (every buffer stays on this rank)");
    std::map<std::pair<int32_t, uint64_t>, const ghx_upack_entry*> by_bytes;  // self pack entries
    std::vector<ghx_upack_entry> src, dst, peers, peer_recv;
    size_t n_self_pack = 0;
    for (const ghx_upack_entry& e : sent)
    {
        if (!self_send[size_t(e.buffer_slot)])
        {
            peers.push_back(e);
            continue;
        }
        by_bytes[{e.buffer_slot, e.buffer_offset}] = &e;
        ++n_self_pack;
    }
    if (by_bytes.size() != n_self_pack)
        return refuse("the self messages' pack and unpack entries do not pair one to one");
    for (const ghx_upack_entry& r : rent)
    {
        const int i = send_of_recv[size_t(r.buffer_slot)];
        if (i < 0)
        {
            peer_recv.push_back(r);
            continue;
        }
        const auto it = by_bytes.find({i, r.buffer_offset});
        if (it == by_bytes.end())
            return refuse("an unpack entry of a self message has no pack entry at the same buffer bytes");
        src.push_back(*it->second);
        dst.push_back(r);
        dst.back().buffer_slot = i;  // a self message's recv buffer IS its send buffer
        by_bytes.erase(it);
    }
    if (!by_bytes.empty())
        return refuse("the self messages' pack and unpack entries do not pair one to one");
    try
    {
        ex.umixed = make_umixed(src.data(), dst.data(), int(src.size()), peers.data(), int(peers.size()));
        if (!peer_recv.empty())
            ex.upunpack = std::make_unique<uplan>(peer_recv.data(), int(peer_recv.size()), 1);
        ex.umixed_reason.clear();
    }
    catch (const invalid& e)
    {
        refuse(e.what());
    }
}
}  // namespace

// The put plan of ghx_cs_put_create (cs_put_plan, k_put_cs): build_cs_self's pairing without the
// buffer. Each target space (dst[k]'s box b with its global box and tile) is matched with the
// source space at the same virtual message bytes and routed by pair_cs_space: pair records or put
// tile records. Throws `invalid` with the reason for what a put cannot serve.
std::unique_ptr<cs_put_plan> build_cs_put(const ghx_pack_entry* src, int n_src,
                                          const ghx_pack_entry* dst, int n_dst,
                                          const ghx_cs_item* cs, const ghx_box* const* global,
                                          const int32_t* const* tiles)
{
    auto check_entry = [](const ghx_pack_entry& e) {
        validate_field(e.field);
        if (e.field.dim - (e.field.has_components ? 1 : 0) != 3)
            throw invalid("a cubed-sphere field has the three spatial dimensions x, y, z");
        if (e.field_slot < 0 || e.buffer_slot < 0) throw invalid("negative slot");
        if (e.field_slot >= GHX_MAX_SLOTS)
            throw invalid("a put plan takes at most 64 source and 64 target fields (one launch)");
        if (e.n_boxes < 0 || (e.n_boxes > 0 && !e.boxes)) throw invalid("bad boxes");
    };
    space_index by_bytes;  // the source spaces by the message bytes they occupy
    size_t n_src_spaces = 0;
    for (int k = 0; k < n_src; ++k)
    {
        const ghx_pack_entry& e = src[k];
        check_entry(e);
        uint64_t off = e.buffer_offset;
        for (int b = 0; b < e.n_boxes; ++b)
        {
            const ghx_box& s = e.boxes[b];
            // below local cell 0 lies the sender's own halo, which its sources may be writing
            if (s.first[0] < 0 || s.first[1] < 0 || s.first[2] < 0)
                throw invalid("a source box reaches into its field's halo (it starts below local cell 0)");
            if (!add_space(by_bytes, e, s, off))
                throw invalid("two source spaces at the same message bytes");
            for (int d = 0; d < 3; ++d)
                if (s.last[d] < s.first[d]) throw invalid("iteration space: first must be <= last");
            off += box_bytes(e, s);
            ++n_src_spaces;
        }
    }
    std::vector<seg_s> from, to;
    std::vector<int32_t> gs, gd;
    std::vector<xsbox> boxes;
    uint64_t bytes = 0;
    size_t n_dst_spaces = 0;
    for (int k = 0; k < n_dst; ++k)
    {
        const ghx_pack_entry& re = dst[k];
        check_entry(re);
        check_cs_item(re.field, cs[k]);
        if (re.n_boxes > 0 && (!global[k] || !tiles[k]))
            throw invalid("a target entry without the global boxes or tiles of its spaces");
        uint64_t off = re.buffer_offset;
        for (int b = 0; b < re.n_boxes; ++b, ++n_dst_spaces)
        {
            const auto it = by_bytes.find({re.buffer_slot, off});
            if (it == by_bytes.end())
                throw invalid("a target space has no source space at the same message bytes");
            is_pair sp{};
            for (int d = 0; d < 3; ++d)
            {
                sp.lf[d] = re.boxes[b].first[d];
                sp.ll[d] = re.boxes[b].last[d];
                sp.gf[d] = global[k][b].first[d];
                sp.gl[d] = global[k][b].last[d];
            }
            // the message is the dense box in the sender's coordinates, which are the global
            // box's: the source box must have its shape (the target's under the transform)
            const ghx_box& sbox = *it->second.box;
            for (int d = 0; d < 3; ++d)
                if (int64_t(sbox.last[d]) - sbox.first[d] != int64_t(sp.gl[d]) - sp.gf[d])
                    throw invalid("a source box and its target box differ in shape under the tile transform");
            const cs_pairing pr = pair_cs_space(*it->second.e, sbox, re, cs[k], sp, tiles[k][b], 0, off);
            for (size_t i = 0; i < pr.from.size(); ++i)
            {
                from.push_back(pr.from[i]);
                to.push_back(pr.to[i]);
                gs.push_back(it->second.e->field_slot);
                gd.push_back(re.field_slot);
            }
            if (!pr.paired) boxes.push_back(pr.box);
            bytes += pr.bytes;
            off += pr.bytes;
        }
    }
    if (n_dst_spaces != n_src_spaces)
        throw invalid("source and target iteration spaces do not describe the same message bytes "
                      "(a source space has no target space)");
    return std::make_unique<cs_put_plan>(from, to, gs, gd, boxes, bytes);
}

// ---------------------------------------------------------------------------------- exchange
// ghx_exchange_create (cs = null) and ghx_cs_exchange_create: with cubed-sphere items the
// receive side is planned space by space (cs_plan_space) into the ordinary unpack plan and the
// transformed one.
std::unique_ptr<ghx_exchange> make_exchange(const ghx_exchange_item* items, const ghx_cs_item* cs,
                                            int32_t n_items)
{
    if (n_items < 1 || !items) throw invalid("need at least one exchange item");
    auto ex = std::make_unique<ghx_exchange>();
    ex->n_items = n_items;
    for (int32_t i = 0; i < n_items; ++i)
    {
        ex->only_unstructured = ex->only_unstructured && !cs && items[i].kind == 1;
        ex->only_structured = ex->only_structured && items[i].kind == 0;
    }
    ex->cubed_sphere = cs != nullptr;
    if (cs)
        for (int32_t i = 0; i < n_items; ++i)
        {
            ex->cs_items.push_back(cs[i]);
            ex->cs_elem.push_back(items[i].field.elem_size);
        }
    std::vector<ghx_pack_entry> rent;              // receive entries, for build_mixed
    std::vector<const halo_entry*> rhalos;         // and their halo entries, for build_cs_self
    for (int dir = 0; dir < 2; ++dir)
    {
        const bool receive = dir == 1;
        std::vector<ghx_pack_entry> sent;
        std::vector<ghx_upack_entry> uent;
        std::vector<std::vector<ghx_box>> store;
        store.reserve(size_t(n_items) * 64);
        auto& bufs = receive ? ex->recv : ex->send;
        std::vector<const halo_entry*> halos;
        plan_direction(items, n_items, receive, bufs, sent, uent, store, &halos);
        // kept for per-buffer plans (ghx_exchange_split); moving the outer vector moves the
        // inner ones, so the entries' box pointers stay valid
        ex->box_store[dir] = std::move(store);
        ex->entries[dir] = sent;
        ex->uentries[dir] = uent;
        if (receive) rent = sent;
        if (receive) rhalos = halos;
        if (receive && cs)
        {
            cs_recv_plan rp;
            for (size_t k = 0; k < sent.size(); ++k)
            {
                const ghx_pack_entry& pe = sent[k];
                const halo_entry& he = *halos[k];
                if (he.tiles.size() != he.boxes.size())
                    throw invalid("cubed-sphere exchange item whose pattern is not a cubed-sphere pattern");
                uint64_t off = pe.buffer_offset;
                for (size_t b = 0; b < he.boxes.size(); ++b)
                {
                    uint64_t nb = 0;
                    cs_plan_space(rp, pe.field, cs[pe.field_slot], he.boxes[b], he.tiles[b],
                                  pe.field_slot, pe.buffer_slot, off, &nb);
                    off += nb;
                }
            }
            ex->cs_rotated = rp.n_rotated;
            ex->cs_segs = rp.segs;  // for the reverse pack (make_cs_adjoint)
            ex->cs_gf = rp.gf;
            ex->cs_gb = rp.gb;
            ex->cs_sbytes = rp.sbytes;
            for (const halo_entry* he : halos)  // for the fused adjoint (make_cs_adjoint_self)
            {
                ex->cs_rhalos.emplace_back();
                ex->cs_rhalos.back().boxes = he->boxes;
                ex->cs_rhalos.back().tiles = he->tiles;
            }
            if (!rp.segs.empty())
                ex->sunpack = std::make_unique<splan>(std::move(rp.segs), rp.gf, rp.gb, rp.sbytes, 1);
            if (!rp.xs.empty()) ex->xunpack = std::make_unique<xplan>(std::move(rp.xs));
            continue;
        }
        if (!sent.empty())
            (receive ? ex->sunpack : ex->spack) =
                std::make_unique<splan>(sent.data(), int(sent.size()), receive ? 1 : 0);
        if (!sent.empty() && g_tune.self_tile_bytes != g_tune.tile_bytes)
        {
            // candidate plans for the fused self exchange (kept only if it is fusable)
            const tile_bytes_scope tile(g_tune.self_tile_bytes);
            (receive ? ex->self_unpack : ex->self_pack) =
                std::make_unique<splan>(sent.data(), int(sent.size()), receive ? 1 : 0);
        }
        if (!uent.empty())
            (receive ? ex->uunpack : ex->upack) =
                std::make_unique<uplan>(uent.data(), int(uent.size()), receive ? 1 : 0);
    }
    ex->self_ok = all_self(*ex);
    if (!ex->self_fusable() || !ex->self_pack || !ex->self_unpack ||
        !exchange_plan::same_messages(*ex->self_pack, *ex->self_unpack))
    {
        ex->self_pack.reset();
        ex->self_unpack.reset();
    }
    if (ex->self_fusable())
    {
        const splan& p = ex->self_pack ? *ex->self_pack : *ex->spack;
        const splan& q = ex->self_unpack ? *ex->self_unpack : *ex->sunpack;
        upload_pair_records(ex->self_recs, p.first().host_segs, q.first().host_segs,
                            p.first().host_tiles);
    }
    // the self messages (make_sadjoint_self): buffer k of both sides when every message is one
    ex->send_of_recv = self_pairs(*ex, items[0].pattern->my_rank);
    if (ex->self_ok)
        for (size_t j = 0; j < ex->recv.size(); ++j) ex->send_of_recv[j] = int(j);
    if (ex->cs_rotated == 0) build_mixed(*ex, items[0].pattern->my_rank, rent);
    if (cs) build_cs_self(*ex, cs, items[0].pattern->my_rank, rhalos);
    else ex->cs_self_reason = "not fusable: not a cubed-sphere exchange";
    build_uself(*ex, items[0].pattern->my_rank);
    build_umixed(*ex, items[0].pattern->my_rank);
    return ex;
}

void exchange_plan::make_split()
{
    if (split) return;
    if (cs_rotated > 0)
        throw invalid("per-buffer plans are not available on a cubed-sphere exchange with "
                      "rotated spaces (the per-buffer unpack does not rotate)");
    for (int dir = 0; dir < 2; ++dir)
    {
        const size_t nb = dir == 0 ? send.size() : recv.size();
        bplan[dir].clear();
        ubplan[dir].clear();
        bplan[dir].resize(nb);
        ubplan[dir].resize(nb);
        for (size_t b = 0; b < nb; ++b)
        {
            std::vector<ghx_pack_entry> se;
            for (const auto& e : entries[dir])
                if (size_t(e.buffer_slot) == b) se.push_back(e);
            std::vector<ghx_upack_entry> ue;
            for (const auto& e : uentries[dir])
                if (size_t(e.buffer_slot) == b) ue.push_back(e);
            if (!se.empty()) bplan[dir][b] = std::make_unique<splan>(se.data(), int(se.size()), dir);
            if (!ue.empty()) ubplan[dir][b] = std::make_unique<uplan>(ue.data(), int(ue.size()), dir);
        }
    }
    split = true;
    for (int dir = 0; dir < 2; ++dir) set_split_parity(dir);
}

namespace
{
using adjoint_kind = exchange_plan::adjoint_kind;

// What every adjoint create refuses of its exchange and arguments: the items the kind does not
// take, double-buffered buffers, and the dtype codes (a receive-only item names no contribution
// entry: its code, and on the cubed sphere its size, is checked here).
void check_adjoint_args(const exchange_plan& ex, adjoint_kind kind, const int32_t* dtypes, int32_t n)
{
    const bool cs = kind == exchange_plan::adj_cs || kind == exchange_plan::adj_cs_self;
    if (kind == exchange_plan::adj_list || kind == exchange_plan::adj_list_self)
    {
        if (!ex.only_unstructured)
            throw invalid("adjoint exchange: the exchange holds a structured or cubed-sphere item (their send "
                          "boxes overlap; only index-list items have an adjoint)");
    }
    else if (cs)
    {
        if (!ex.cubed_sphere)
            throw invalid("cubed-sphere adjoint exchange: not a cubed-sphere exchange (regular structured items take "
                          "ghx_sexchange_adjoint_create, index-list items ghx_uexchange_adjoint_create)");
    }
    else
    {
        if (ex.cubed_sphere)
            throw invalid(std::string("adjoint exchange: the exchange holds a cubed-sphere item (its adjoint would "
                                      "rotate and flip signs; only regular structured items take ") +
                          (kind == exchange_plan::adj_boxes ? "ghx_sexchange_adjoint_create)"
                                                            : "ghx_sexchange_adjoint_self_create)"));
        if (!ex.only_structured)
            throw invalid("adjoint exchange: the exchange holds an unstructured item (an exchange mixing structured "
                          "and unstructured items has no adjoint; index-list items take ghx_uexchange_adjoint_create)");
    }
    ex.check_single_buffered();
    if (n != ex.n_items || !dtypes) throw invalid("adjoint exchange: one dtype code per exchange item");
    for (int32_t i = 0; i < n; ++i)
    {
        if (dtypes[i] < GHX_DT_F32 || dtypes[i] > GHX_DT_I64)
            throw invalid("unknown dtype code " + std::to_string(dtypes[i]) + " (GHX_DT_F32, _F64, _I32, _I64)");
        if (!cs) continue;
        const int32_t size = (dtypes[i] == GHX_DT_F32 || dtypes[i] == GHX_DT_I32) ? 4 : 8;
        if (size != ex.cs_elem[size_t(i)])
            throw invalid("cubed-sphere adjoint exchange: item " + std::to_string(i) + " has dtype code " +
                          std::to_string(dtypes[i]) + " (" + std::to_string(size) + " B) but elem_size " +
                          std::to_string(ex.cs_elem[size_t(i)]));
        const ghx_cs_item& item = ex.cs_items[size_t(i)];
        const int32_t value_kind = dtypes[i] <= GHX_DT_F64 ? 1 : 2;
        if (item.is_vector && item.value_kind != value_kind)
            throw invalid("cubed-sphere adjoint exchange: vector item " + std::to_string(i) + " has value_kind " +
                          std::to_string(item.value_kind) + " but dtype code " + std::to_string(dtypes[i]) +
                          " (1: GHX_DT_F32 / _F64, 2: GHX_DT_I32 / _I64)");
    }
}

// The self messages of an exchange, entry by entry: the receive entry at the same message bytes
// sources a self message's send entry.
struct self_match
{
    std::vector<int> recv_of;  // per send entry: its receive entry, -1 for a peer message's
    std::vector<size_t> peer;  // the receive entries of the peer messages
    size_t n_self = 0;
};

// throws unless every entry of a self message has its counterpart and there is a self message;
// `plain_create` names the create that serves an exchange without one. se / re: the send and
// receive entries, of boxes or of lists
template<typename Entry>
self_match match_self_messages(const exchange_plan& ex, const std::vector<Entry>& se, const std::vector<Entry>& re,
                               const char* plain_create)
{
    std::vector<int> recv_of_send(ex.send.size(), -1);
    for (size_t j = 0; j < ex.send_of_recv.size(); ++j)
        if (ex.send_of_recv[j] >= 0) recv_of_send[size_t(ex.send_of_recv[j])] = int(j);
    self_match m;
    std::vector<char> sourced(re.size(), 0);
    for (const Entry& e : se)
    {
        m.recv_of.push_back(-1);
        const int j = recv_of_send[size_t(e.buffer_slot)];
        if (j < 0) continue;
        for (size_t k = 0; k < re.size() && m.recv_of.back() < 0; ++k)
            if (re[k].buffer_slot == j && re[k].buffer_offset == e.buffer_offset) m.recv_of.back() = int(k);
        if (m.recv_of.back() < 0)
            throw invalid("fused adjoint: a send entry of a self message has no receive entry at the same "
                          "message bytes");
        sourced[size_t(m.recv_of.back())] = 1;
        ++m.n_self;
    }
    if (m.n_self == 0)
        throw invalid(std::string("fused adjoint: the exchange has no self message (") + plain_create + ")");
    for (size_t k = 0; k < re.size(); ++k)
    {
        if (sourced[k]) continue;
        if (ex.send_of_recv[size_t(re[k].buffer_slot)] >= 0)
            throw invalid("fused adjoint: a receive entry of a self message has no send entry at the same "
                          "message bytes");
        m.peer.push_back(k);
    }
    return m;
}
}  // namespace

void exchange_plan::check_single_buffered() const
{
    if (dir_parity[0].word || dir_parity[1].word)
        throw invalid("adjoint exchange: the exchange has double-buffered buffers "
                      "(ghx_exchange_set_parity); its launches use one copy");
}

void exchange_plan::make_adjoint(adjoint_kind kind, const int32_t* dtypes, int32_t n)
{
    check_adjoint_args(*this, kind, dtypes, n);
    adjoint_set set;
    set.form = 1;
    if (kind == adj_list)
    {
        std::vector<int32_t> dt;
        for (const ghx_upack_entry& e : uentries[0]) dt.push_back(dtypes[e.field_slot]);
        set.uaccum = std::make_unique<uaccum_plan>(uentries[0].data(), dt.data(), int(dt.size()), uentries[1].data(),
                                                   int(uentries[1].size()));
        set.upack = std::make_unique<uplan>(uentries[1].data(), int(uentries[1].size()), 0);
        adjoint[kind] = std::move(set);
        return;
    }
    if (kind == adj_list_self)
    {
        const std::vector<ghx_upack_entry>&se = uentries[0], &re = uentries[1];
        const self_match m = match_self_messages(*this, se, re, "ghx_uexchange_adjoint_create");
        std::vector<int32_t> dt;
        std::vector<const ghx_upack_entry*> source(se.size(), nullptr);
        for (size_t e = 0; e < se.size(); ++e)
        {
            dt.push_back(dtypes[se[e].field_slot]);
            if (m.recv_of[e] >= 0) source[e] = &re[size_t(m.recv_of[e])];
        }
        set.uaccum = std::make_unique<uaccum_plan>(se.data(), dt.data(), int(dt.size()), re.data(), int(re.size()),
                                                   source.data());
        // the reverse pack of the peer receive entries alone
        if (!m.peer.empty())
        {
            std::vector<ghx_upack_entry> peer;
            for (size_t k : m.peer) peer.push_back(re[k]);
            set.upack = std::make_unique<uplan>(peer.data(), int(peer.size()), 0);
        }
        set.form = m.n_self == se.size() && m.peer.empty() ? 1 : 2;
        adjoint[kind] = std::move(set);
        return;
    }
    const std::vector<ghx_pack_entry>&se = entries[0], &re = entries[1];
    std::vector<int32_t> dt;
    for (const ghx_pack_entry& e : se) dt.push_back(dtypes[e.field_slot]);
    auto accum = [&](const ghx_pack_entry* const* source, const xseg* const* space) {
        return std::make_unique<::ghx_saccum>(se.data(), dt.data(), int(dt.size()), re.data(), int(re.size()), source,
                                             space);
    };
    if (kind == adj_boxes)
    {
        set.saccum = accum(nullptr, nullptr);
        set.spack = std::make_unique<splan>(re.data(), int(re.size()), 0);
    }
    else if (kind == adj_cs)
    {
        set.saccum = accum(nullptr, nullptr);
        if (!cs_segs.empty()) set.spack = std::make_unique<splan>(cs_segs, cs_gf, cs_gb, cs_sbytes, 0);
        set.xpack = xunpack.get();
    }
    else
    {
        const bool cs = kind == adj_cs_self;
        const self_match m =
            match_self_messages(*this, se, re, cs ? "ghx_cs_exchange_adjoint_create" : "ghx_sexchange_adjoint_create");
        std::vector<const ghx_pack_entry*> source(se.size(), nullptr);
        // cubed sphere: the receiving side of each box of a paired entry, box k of one with box k of
        // the other as build_cs_self pairs them
        std::vector<std::vector<xseg>> spaces(se.size());
        std::vector<const xseg*> space(se.size(), nullptr);
        for (size_t e = 0; e < se.size(); ++e)
        {
            if (m.recv_of[e] < 0) continue;
            const ghx_pack_entry& r = re[size_t(m.recv_of[e])];
            source[e] = &r;
            if (!cs) continue;
            const halo_entry& he = cs_rhalos[size_t(m.recv_of[e])];
            if (int(he.boxes.size()) != r.n_boxes || r.n_boxes != se[e].n_boxes)
                throw invalid("fused adjoint: contribution entry " + std::to_string(e) +
                              " and its source differ in their number of boxes");
            for (size_t b = 0; b < he.boxes.size(); ++b)
                spaces[e].push_back(cs_space_box(r.field, cs_items[size_t(r.field_slot)], he.boxes[b], he.tiles[b],
                                                 r.field_slot, r.buffer_slot, 0));
            space[e] = spaces[e].data();
        }
        set.saccum = accum(source.data(), cs ? space.data() : nullptr);
        // the reverse pack of the peer receive entries alone
        if (!cs && !m.peer.empty())
        {
            std::vector<ghx_pack_entry> peer;
            for (size_t k : m.peer) peer.push_back(re[k]);
            set.spack = std::make_unique<splan>(peer.data(), int(peer.size()), 0);
        }
        // cubed sphere: the kept ordinary segments and the transformed boxes whose receive buffer
        // is a peer's
        if (cs && !m.peer.empty())
        {
            std::vector<char> peer_buf(recv.size(), 0);
            for (size_t k : m.peer) peer_buf[size_t(re[k].buffer_slot)] = 1;
            std::vector<seg_s> segs;
            std::vector<int32_t> gf, gb;
            uint64_t bytes = 0;
            for (size_t i = 0; i < cs_segs.size(); ++i)
                if (peer_buf[size_t(cs_gb[i])])
                {
                    segs.push_back(cs_segs[i]);
                    gf.push_back(cs_gf[i]);
                    gb.push_back(cs_gb[i]);
                    bytes += cs_segs[i].bytes;
                }
            if (!segs.empty()) set.spack = std::make_unique<splan>(std::move(segs), gf, gb, bytes, 0);
            std::vector<xseg> boxes;
            if (xunpack)
                for (const xseg& b : xunpack->boxes)
                    if (peer_buf[size_t(b.buf_slot)]) boxes.push_back(b);
            if (!boxes.empty()) set.own_xpack = std::make_unique<xplan>(std::move(boxes));
            set.xpack = set.own_xpack.get();
        }
        set.form = m.n_self == se.size() && m.peer.empty() ? 1 : 2;
    }
    adjoint[kind] = std::move(set);
}

int exchange_plan::adjoint_set::pack(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const
{
    int rc = GHX_OK;
    if (upack) rc = upack->execute(fptr, nf, bptr, nb, stream);
    else if (spack) rc = spack->execute(fptr, nf, bptr, nb, stream);
    if (rc == GHX_OK && xpack) rc = xpack->execute_pack(fptr, nf, bptr, nb, stream);
    return rc;
}

int exchange_plan::adjoint_set::accumulate(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos,
                                           void* stream) const
{
    if (uaccum)
        return uaccum->get ? uaccum->execute_get(fptr, nf, bptr, nb, zero_halos, stream)
                           : uaccum->execute(fptr, nf, bptr, nb, zero_halos, stream);
    return saccum->get ? saccum->execute_get(fptr, nf, bptr, nb, zero_halos, stream)
                       : saccum->execute(fptr, nf, bptr, nb, zero_halos, stream);
}

int exchange_plan::execute_buffer(int dir, int b, void* const* fptr, int nf, void* const* bptr,
                                  int nb, void* stream) const
{
    if (!split) throw invalid("exchange is not split (ghx_exchange_split)");
    const size_t n = dir == 0 ? send.size() : recv.size();
    if (b < 0 || size_t(b) >= n) throw invalid("buffer index out of range");
    if (nb < int(n)) throw invalid("too few buffers");
    int rc = GHX_OK;
    if (bplan[dir][size_t(b)]) rc = bplan[dir][size_t(b)]->execute(fptr, nf, bptr, nb, stream);
    if (rc == GHX_OK && ubplan[dir][size_t(b)])
        rc = ubplan[dir][size_t(b)]->execute(fptr, nf, bptr, nb, stream);
    return rc;
}

int exchange_plan::execute_self(void* const* fptr, int nf, void* const* bptr, int nb,
                                void* stream) const
{
    const splan& p = self_pack ? *self_pack : *spack;
    const splan& q = self_unpack ? *self_unpack : *sunpack;
    // the launch reads the pack segments' field slots AND the unpack segments' (a domain
    // that only receives has a field slot no pack segment names, possibly the highest)
    const int nfs = std::max(p.max_field_slot, q.max_field_slot);
    if (nf <= nfs || nb <= p.max_buf_slot) throw invalid("pointer arrays do not cover the plan's slots");
    return launch_paired(launch_self, p.first(), q.first().dev.segs, self_recs.recs, fptr, nfs + 1,
                         "field", bptr, p.max_buf_slot + 1, "buffer", nullptr, stream);
}

int exchange_plan::execute_pack_self(void* const* fptr, int nf, void* const* bptr, int nb,
                                     void* stream) const
{
    const splan& p = *spack;
    // the self messages' unpack (companion) segments name receiving fields too
    const int nfs = std::max(p.max_field_slot, mixed_max_field_slot);
    if (nf <= nfs || nb <= p.max_buf_slot) throw invalid("pointer arrays do not cover the plan's slots");
    return launch_paired(launch_self, p.first(), mixed_comp.segs, mixed_recs.recs, fptr, nfs + 1,
                         "field", bptr, p.max_buf_slot + 1, "buffer", &mixed_parity, stream);
}
}  // namespace ghx

ghx_put::ghx_put(const ghx_pack_entry* src, int n_src, const ghx_pack_entry* dst, int n_dst)
: from(new ghx::splan(src, n_src, 0)), to(new ghx::splan(dst, n_dst, 1))
{
    const std::vector<ghx::seg_s>&fs = from->first().host_segs, &ts = to->first().host_segs;
    bool ok = fs.size() == ts.size() && from->bytes == to->bytes;
    for (size_t k = 0; ok && k < fs.size(); ++k)
    {
        ok = ghx::exchange_plan::same_message(fs[k], ts[k]) && fs[k].n_outer == ts[k].n_outer;
        for (int d = 0; ok && d < 4; ++d) ok = fs[k].ext[d] == ts[k].ext[d];
    }
    if (!ok)
        throw ghx::invalid("source and target iteration spaces do not describe the same "
                           "message bytes (shapes, order, element sizes or row structure differ)");
    if (from->grouped() || to->grouped())
        throw ghx::invalid("a put plan takes at most 64 source and 64 target fields (one launch)");
    ghx::upload_pair_records(recs, fs, ts, from->first().host_tiles);
}

ghx_put::ghx_put(std::unique_ptr<ghx::cs_put_plan> p) : cs(std::move(p)) {}

ghx_put::ghx_put(std::unique_ptr<ghx::uput_plan> p) : u(std::move(p)) {}

int ghx_put::execute(void* const* src, int ns, void* const* dst, int nd, void* stream) const
{
    if (cs) return cs->execute(src, ns, dst, nd, stream);
    if (u) return u->execute(src, ns, dst, nd, stream);
    const ghx::splan& p = *from;
    const ghx::splan& q = *to;
    if (p.first().n_tiles == 0) return GHX_OK;
    if (ns <= p.max_field_slot || nd <= q.max_field_slot)
        throw ghx::invalid("pointer arrays do not cover the plan's slots");
    return ghx::launch_paired(ghx::launch_put, p.first(), q.first().dev.segs, recs.recs, src,
                              p.max_field_slot + 1, "source field", dst, q.max_field_slot + 1,
                              "target field", nullptr, stream);
}
