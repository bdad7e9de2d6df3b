// ghx_exchange.hpp — the exchange plan behind the opaque ghx_exchange handle
// (communication_object::allocate semantics, include/ghex/communication_object.hpp:483-566,
// 1003-1067) and the put plan behind ghx_put, shared by the C ABI (ghx_abi.cpp) and the per-peer
// pipeline (ghx_pipeline.cpp); ghx_exchange.cpp plans and executes them.
#pragma once

#include <memory>
#include <vector>

#include "ghx_pattern.hpp"
#include "ghx_plan.hpp"

namespace ghx
{
struct xbuffer
{
    int32_t first_id, second_id, rank, tag;
    uint64_t size = 0;
};

struct exchange_plan
{
    std::vector<xbuffer> send, recv;
    std::unique_ptr<splan> spack, sunpack;
    std::unique_ptr<uplan> upack, uunpack;
    // the fused self exchange's own pack/unpack plans when its tile size differs from the
    // two-launch path's (g_tune.self_tile_bytes); null = use spack/sunpack
    std::unique_ptr<splan> self_pack, self_unpack;
    // exchanges with self AND peer messages (build_mixed): per segment of spack the unpack
    // segment of its self message (zero = a peer message: pack only), and the unpack plan of
    // the peer messages alone
    device_tables mixed_comp;
    // pair records of the fused launches (upload_pair_records): the all-self exchange's
    // (ghx_exchange_self) and the mixed pack's (ghx_exchange_pack_self); empty: tile table path
    device_tables self_recs, mixed_recs;
    int mixed_max_field_slot = -1;  // the highest field slot mixed_comp's segments name
    std::unique_ptr<splan> punpack;
    bool mixed = false;
    parity_cfg mixed_parity;  // the mixed pack launch's double-buffered send buffers (direct)
    parity_cfg dir_parity[2];  // ghx_exchange_set_parity per direction (the per-buffer plans too)
    int32_t n_items = 0;
    bool self_ok = false;  // may pack and unpack be fused (all self)? Set by make_exchange.

    // The planner's entries per direction (0 send, 1 recv), kept for per-buffer plans; boxes
    // point into box_store, unstructured lids into the pattern (which outlives the exchange,
    // include/ghex/pattern_container.hpp:84-87).
    std::vector<ghx_pack_entry> entries[2];
    std::vector<std::vector<ghx_box>> box_store[2];
    std::vector<ghx_upack_entry> uentries[2];
    // per-buffer plans (ghx_exchange_split): [direction][buffer index], null = no bytes of
    // that kind in that buffer. The reference packs each buffer on its own stream
    // (include/ghex/communication_object.hpp:568-597, device/cuda/stream.hpp:25-73).
    std::vector<std::unique_ptr<splan>> bplan[2];
    std::vector<std::unique_ptr<uplan>> ubplan[2];
    bool split = false;
    // cubed sphere (ghx_cs_exchange_create): the transformed unpack launch, and the number of
    // rotated receive spaces (those planned as ordinary segments included). With one rotated
    // space the exchange is neither fused, mixed nor split: those paths unpack from `entries`,
    // which know nothing of the rotation.
    std::unique_ptr<xplan> xunpack;
    int32_t cs_rotated = 0;
    // the fused self exchange of a cubed-sphere exchange whose every message stays on this rank
    // (ghx_cs_exchange_self): null when it cannot be fused, cs_self_reason then says why
    std::unique_ptr<cs_self_plan> cs_self;
    std::string cs_self_reason;
    // the fused self exchange of an exchange of unstructured items whose every message stays on
    // this rank (ghx_uexchange_self, k_self_u): null when it cannot be fused, uself_reason says why
    std::unique_ptr<uput_plan> uself;
    std::string uself_reason;
    // an exchange of unstructured items with self AND peer messages (ghx_uexchange_pack_self,
    // k_pack_self_u): the pack plan that also completes the self messages, and the unpack plan of
    // the peer messages alone (null: the rank receives from no peer). umixed is null when the
    // form does not apply, umixed_reason then says why
    std::unique_ptr<uput_plan> umixed;
    std::unique_ptr<uplan> upunpack;
    std::string umixed_reason;
    // The adjoint of the exchange: one plan set per kind, created on demand by
    // make_adjoint and independent of each other (the plain and the fused form of one exchange
    // coexist). The reverse pack gathers the halo cells into the receive buffers, the accumulate
    // adds the send buffers' contributions into their owners.
    //  list (ghx_uexchange_adjoint_create): a pack plan over uentries[1]; k_accum_u with uentries[0]
    //   as contribution entries and uentries[1] as zero entries.
    //  boxes (ghx_sexchange_adjoint_create): the same over entries[1] and entries[0] (k_accum_s).
    //  boxes_self (ghx_sexchange_adjoint_self_create): the self messages fused. The get plan
    //   (k_accum_get_s) reads a self message from the receiving field's halo cells, and the reverse
    //   pack covers the peer receive entries alone.
    //  cs (ghx_cs_exchange_adjoint_create): the reverse pack is the transpose of the unpack in its two
    //   parts: a pack plan over the ordinary receive segments (cs_segs: a copy of what sunpack was
    //   built from) and k_pack_x over xunpack's own records (no second tiler, no second upload). The
    //   accumulate plan is that of boxes: the send side of a cubed-sphere exchange is ordinary boxes
    //   of the sender's field.
    //  cs_self (ghx_cs_exchange_adjoint_self_create): the get plan (k_accum_get_x) reads a self message
    //   from the receiving field's halo cells through the edge's transform, and the reverse pack
    //   covers the peer receive spaces alone: the kept ordinary segments and xunpack's boxes filtered
    //   by receive buffer.
    //  list_self (ghx_uexchange_adjoint_self_create): list with the self messages fused. The get plan
    //   (k_accum_get_u) reads a self message from the receiving field's halo cells, and the reverse
    //   pack covers the peer receive entries alone.
    enum adjoint_kind { adj_list, adj_boxes, adj_boxes_self, adj_cs, adj_cs_self, adj_list_self, n_adjoint_kinds };
    struct adjoint_set
    {
        // 0 not created; 1 created (a fused set: every message is a self message); 2 a fused set
        // with self and peer messages
        int32_t form = 0;
        // the reverse pack: at most one ordinary plan and at most one transformed pack, which the
        // set owns (cs_self) or borrows from the exchange's xunpack (cs). All null: nothing to gather
        std::unique_ptr<splan> spack;
        std::unique_ptr<uplan> upack;
        std::unique_ptr<xplan> own_xpack;
        const xplan* xpack = nullptr;
        // the accumulate plan: uaccum for list and list_self, else saccum (the handle type: the
        // cubed-sphere *_plan calls lend it); a get plan in the fused sets
        std::unique_ptr<uaccum_plan> uaccum;
        std::unique_ptr<::ghx_saccum> saccum;
        // the ordinary launch, then the transformed one on the same stream
        int pack(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;
        int accumulate(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const;
    };
    adjoint_set adjoint[n_adjoint_kinds];
    // throws `invalid` and leaves adjoint[kind] as it was
    void make_adjoint(adjoint_kind kind, const int32_t* dtypes, int32_t n);
    // both launches of an adjoint use one copy of each buffer: its creates and launches refuse an
    // exchange with double-buffered buffers (ghx_exchange_set_parity)
    void check_single_buffered() const;
    bool only_unstructured = true;  // every item is an index-list item (set by make_exchange)
    bool only_structured = true;  // every item is a regular structured item (set by make_exchange)
    bool cubed_sphere = false;    // made by ghx_cs_exchange_create
    // send_of_recv: per recv buffer the send buffer of the same self message or -1 (self_pairs,
    // the match of build_mixed), set by make_exchange.
    std::vector<int> send_of_recv;
    // cubed sphere: the ordinary receive segments with their caller slots and bytes, the items with
    // their element sizes, and cs_rhalos: a copy of the halo entry (boxes in both coordinates,
    // tiles) behind each of entries[1], kept by make_exchange
    std::vector<seg_s> cs_segs;
    std::vector<int32_t> cs_gf, cs_gb;
    uint64_t cs_sbytes = 0;
    std::vector<ghx_cs_item> cs_items;  // per item, with its element size
    std::vector<int32_t> cs_elem;
    std::vector<halo_entry> cs_rhalos;

    void make_split();  // the per-buffer plans (ghx_exchange_split)

    // the per-buffer plans use the copies ghx_exchange_set_parity selected, like the whole ones
    void set_split_parity(int dir)
    {
        for (auto& p : bplan[dir])
            if (p) p->parity = dir_parity[dir];
        for (auto& p : ubplan[dir])
            if (p) p->parity = dir_parity[dir];
    }

    // one buffer's pack (dir 0) or unpack (dir 1); the pointer arrays are the whole exchange's
    int execute_buffer(int dir, int b, void* const* fptr, int nf, void* const* bptr, int nb,
                       void* stream) const;

    // Every recv buffer aliases the send buffer of the same pair, and pack segment k and unpack
    // segment k cover the same buffer bytes (the launch tiles by the pack plan's table).
    bool self_fusable() const { return self_ok; }
    // the fused launches: the all-self exchange (ghx_exchange_self) and the mixed pack
    // (ghx_exchange_pack_self), k_self over the pack plan's tiles
    int execute_self(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;
    int execute_pack_self(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;

    // Segment a of a launch's primary plan and its companion b (the unpack side of a fused self
    // tile, the target side of a put) cover the same buffer bytes with the same rows. Tiling is
    // deliberately not compared: a fused launch (k_self, k_put) runs the primary plan's tile
    // table and reads only a's tile_bytes, and the two sides size their short-row tiles from
    // different fields' row counts (a put's one source field vs one target field per peer; the
    // mixed pairing's self messages vs every message of the field), which differ once a field
    // holds more than the 512-row minimum's worth (512^3 (2,2,1) puts refused).
    static bool same_message(const seg_s& a, const seg_s& b)
    {
        return a.buf_slot == b.buf_slot && a.buf_off == b.buf_off && a.bytes == b.bytes &&
               a.row_bytes == b.row_bytes;
    }

    // pack segment k and unpack segment k cover the same buffer bytes (same_message)
    static bool same_messages(const splan& p, const splan& q)
    {
        const std::vector<seg_s>&a = p.first().host_segs, &b = q.first().host_segs;
        bool ok = a.size() == b.size();
        for (size_t k = 0; ok && k < a.size(); ++k) ok = same_message(a[k], b[k]);
        return ok;
    }
};
}  // namespace ghx

struct ghx_exchange : ghx::exchange_plan
{
};

// Put plan: the pack plan of the source side and the unpack plan of the target side, segment k
// of each covering the same virtual message bytes (checked). The launch is tiled by the source
// plan's tile table alone (k_put addresses the target segment by message position), so the
// target plan's own tiling is not compared: the two sides size their short-row tiles by their
// own fields' rows (one source field, one target field per peer) and differ at large sizes.
struct ghx_put
{
    std::unique_ptr<ghx::splan> from, to;
    ghx::device_tables recs;  // pair records (source segment with tile index, target segment)
    // a put made by ghx_cs_put_create: `cs` alone (pair records and put tile records, k_put_cs)
    std::unique_ptr<ghx::cs_put_plan> cs;
    // a put made by ghx_uput_create: `u` alone (index-list tile records, k_put_u)
    std::unique_ptr<ghx::uput_plan> u;
    ghx_put(const ghx_pack_entry* src, int n_src, const ghx_pack_entry* dst, int n_dst);
    explicit ghx_put(std::unique_ptr<ghx::cs_put_plan> p);
    explicit ghx_put(std::unique_ptr<ghx::uput_plan> p);
    int execute(void* const* src, int ns, void* const* dst, int nd, void* stream) const;
};

// The plan of ghx_uself_create: an index-list put plan with its buffer side (ghx::make_uself)
struct ghx_uself
{
    std::unique_ptr<ghx::uput_plan> p;
};

namespace ghx
{
// ghx_exchange_create (cs = null) and ghx_cs_exchange_create (one cubed-sphere item per item)
std::unique_ptr<ghx_exchange> make_exchange(const ghx_exchange_item* items, const ghx_cs_item* cs,
                                            int32_t n_items);
// the put plan of ghx_cs_put_create; throws `invalid` with the reason for what a put cannot serve
std::unique_ptr<cs_put_plan> build_cs_put(const ghx_pack_entry* src, int n_src,
                                          const ghx_pack_entry* dst, int n_dst, const ghx_cs_item* cs,
                                          const ghx_box* const* global, const int32_t* const* tiles);
}  // namespace ghx
