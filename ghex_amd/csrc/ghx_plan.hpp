// ghx_plan.hpp — host planner objects behind the opaque C handles.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "ghx_internal.hpp"

namespace ghx
{
struct invalid : std::runtime_error
{
    using std::runtime_error::runtime_error;
};
struct hip_error : std::runtime_error
{
    using std::runtime_error::runtime_error;
};

struct device_tables
{
    void* segs = nullptr;
    uint32_t* tiles = nullptr;
    void* recs = nullptr;  // tile records (g_tune.tile_records): per tile a copy of its segment
    void* lids = nullptr;
    void release();
    device_tables() = default;
    device_tables(const device_tables&) = delete;
    device_tables& operator=(const device_tables&) = delete;
    ~device_tables() { release(); }
};

void validate_field(const ghx_field_desc& f);
// segment table alone to device memory (a no-op without a HIP device)
void upload_segments(device_tables& dt, const std::vector<seg_s>& segs);
// Pair records of a fused launch (k_self, k_put; g_tune.tile_records): per tile of the primary
// plan, in its dispatch order, the primary segment (with the tile's index in first_tile) and
// the companion segment of the same index, side by side (dt.recs; a no-op without a device or
// with tile_records off); pair_records builds the table on the host
std::vector<seg_s> pair_records(const std::vector<seg_s>& primary, const std::vector<seg_s>& companion,
                                const std::vector<uint32_t>& tiles);
void upload_pair_records(device_tables& dt, const std::vector<seg_s>& primary,
                         const std::vector<seg_s>& companion, const std::vector<uint32_t>& tiles);
uint64_t add_box_segments(std::vector<seg_s>& out, const ghx_field_desc& f, const ghx_box& box,
                          uint16_t field_slot, uint16_t buf_slot, uint64_t buf_off);
// plans built inside its scope tile their long rows by `bytes` (g_tune.tile_bytes, put back on
// every exit)
struct tile_bytes_scope
{
    const uint32_t saved = g_tune.tile_bytes;
    explicit tile_bytes_scope(uint32_t bytes) { g_tune.tile_bytes = bytes; }
    ~tile_bytes_scope() { g_tune.tile_bytes = saved; }
};
// the derived members of a segment built by hand (divisors, vector width, addressing form) from
// its offsets, strides, extents, row length and byte count
void finish_segment(seg_s& s);

// Launch groups. A launch carries at most GHX_MAX_SLOTS field and buffer pointers (kargs is
// passed by value); a plan whose entries use more slots than that (many fields in one exchange,
// or many domain-pair buffers: a rank holding many domains) is cut into groups of segments in
// entry order, each with its own slot maps (local slot -> the caller's slot) and tables, and
// executes as one launch per group on the same stream. The reference has no such limit
// (include/ghex/communication_object.hpp:1003-1067 allocates any number of buffers).
// Every plan holds all its groups in `groups`; a plan without segments has one empty group.
template<typename Seg>
struct launch_group
{
    std::vector<int32_t> fmap, bmap;   // local slot -> caller slot; empty: identity
    uint32_t n_tiles = 0;
    std::vector<Seg> host_segs;        // local slots (xplan: its tile records)
    std::vector<uint32_t> host_tiles;  // the tile table (pair records)
    device_tables dev;
};
template<typename Seg>
uint32_t total_tiles(const std::vector<launch_group<Seg>>& groups)
{
    uint32_t t = 0;
    for (const auto& g : groups) t += g.n_tiles;
    return t;
}
template<typename Seg>
bool grouped(const std::vector<launch_group<Seg>>& groups)
{
    return groups.size() > 1 || !groups[0].fmap.empty() || !groups[0].bmap.empty();
}
// Fill a launch's pointer slots from the caller's arrays through a group's maps (empty: the
// first n_identity pointers as they are); `what` names the pointers in the null refusal.
void fill_slots(uint64_t* dst, void* const* src, const std::vector<int32_t>& map, int n_identity,
                const char* what);

// structured fused plan
struct splan
{
    int direction = 0;
    uint64_t bytes = 0;
    int32_t n_segments = 0;
    uint32_t tile_bytes = kTileBytes;
    int max_field_slot = -1, max_buf_slot = -1;  // caller slots
    std::vector<launch_group<seg_s>> groups;
    parity_cfg parity;                           // double-buffered buffers (direct exchange)
    bool grouped() const { return ghx::grouped(groups); }
    uint32_t total_tiles() const { return ghx::total_tiles(groups); }
    // the one group of a plan that is not grouped() (the fused launches take no other)
    const launch_group<seg_s>& first() const { return groups[0]; }
    splan(const ghx_pack_entry* entries, int n_entries, int direction);
    // from ready segments (cubed sphere: rotated spaces that keep contiguous rows): gf / gb are
    // the caller's field / buffer slot of each segment, `bytes` the buffer bytes they cover
    splan(std::vector<seg_s> segs, const std::vector<int32_t>& gf, const std::vector<int32_t>& gb,
          uint64_t bytes, int direction);
    int execute(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;
};

// transformed unpack plan (cubed sphere): the tile records of its xseg boxes, cut into launch
// groups of at most GHX_MAX_SLOTS field and buffer slots like the other plans. One k_unpack_x
// launch per group, enqueued after the ordinary unpack launch on the same stream.
struct xplan
{
    uint64_t bytes = 0;
    int32_t n_records = 0;     // boxes
    uint32_t n_tiles = 0;      // of all groups
    int max_field_slot = -1, max_buf_slot = -1;  // caller slots
    std::vector<xseg> boxes;
    std::vector<launch_group<seg_x>> groups;  // host_segs: the tile records, dev.recs on the device
    explicit xplan(std::vector<xseg> boxes);
    int execute(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;
    // the transpose (k_pack_x): the same records and tables, receiving field -> buffer
    int execute_pack(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;
};
// where a tile record lies in its box: the tile's origin per BUFFER axis of the xseg, and the
// buffer axis each of the record's (stride-sorted) axes is
struct xtile_pos
{
    uint32_t origin[4];
    int32_t axis[4];
};
// the tile records of one box (local slots as given); `where`, if given, gains one entry per record
void make_tile_records(std::vector<seg_x>& out, const xseg& b, uint16_t field_slot,
                       uint16_t buf_slot, std::vector<xtile_pos>* where = nullptr);

// Fused cubed-sphere self exchange (k_self_cs): every message of the exchange is
// a self message, so ONE launch reads each sent cell from the sending field and writes it to the
// send buffer and to the receiving field's halo. Receive spaces whose unpack segments cover the
// same bytes with the same rows as the pack segments become pair records (as k_self's); every
// other space becomes self tile records (seg_xs). Built without a device; the records are kept on
// the host for inspection and uploaded when there is a device.
struct xsbox
{
    xseg dst;               // the receiving side (slots: the receiving field's, the buffer's)
    int64_t src_off;        // sending field: byte offset of buffer cell (0, 0, 0, 0)
    int64_t src_stride[4];  // and its byte stride per buffer axis
    int32_t src_slot;
};
// the two record tables of a cubed-sphere launch (k_self_cs, k_put_cs) and how they are built
struct cs_records
{
    std::vector<seg_s> pair_recs;  // two per pair tile: the pack / source segment (first_tile =
                                   // the tile's index in it), then the unpack / target segment
    std::vector<seg_xs> x_recs;    // one per self / put tile
    int32_t n_x_records = 0;       // spaces (boxes) behind x_recs
    device_tables dev;             // dev.segs: pair_recs, dev.recs: x_recs
    uint32_t n_pair_tiles() const { return uint32_t(pair_recs.size() / 2); }
    uint32_t n_x_tiles() const { return uint32_t(x_recs.size()); }

protected:
    void build_pairs(std::vector<seg_s> primary, std::vector<seg_s> companion);  // slots set
    void build_tiles_x(const std::vector<xsbox>& boxes, bool buffered);
    void upload(const char* what);
    void check_tables() const;  // throws when a launch would lack its device tables
};
struct cs_self_plan : cs_records
{
    int max_field_slot = -1, max_buf_slot = -1;
    // pack / unpack segments of the paired spaces (segment k of each over the same bytes, caller
    // slots gf_p / gf_u / gb) and the boxes of the others
    cs_self_plan(const std::vector<seg_s>& pack, const std::vector<seg_s>& unpack,
                 const std::vector<int32_t>& gf_p, const std::vector<int32_t>& gf_u,
                 const std::vector<int32_t>& gb, const std::vector<xsbox>& boxes);
    int execute(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;
};

// Cubed-sphere put (k_put_cs): the zero-copy form of the walk above. Spaces whose
// source and target segments cover the same message bytes with the same rows become pair records
// and run as k_put runs them; every other space becomes put tile records: seg_xs whose buffer
// side (x.buf_off, x.buf_slot, x.bstride) is unused — each lane loads one element from the
// sending field and stores it, negated as `x` says, to the receiving field, which may be a peer's
// IPC-mapped memory. Field slots: the sender's (pair primary, seg_xs::src_slot) index the
// source pointer array, the receiver's (pair companion, x.field_slot) the target pointer array;
// fewer than GHX_MAX_SLOTS of each (one launch). Built without a device like cs_self_plan.
struct cs_put_plan : cs_records
{
    uint64_t bytes = 0;            // message bytes moved per execution
    int max_src_slot = -1, max_dst_slot = -1;
    // source / target segments of the paired spaces (segment k of each over the same message
    // bytes; gs / gd: the source / target field slot of each) and the boxes of the others
    // (dst.field_slot: the target slot, src_slot: the source slot)
    cs_put_plan(const std::vector<seg_s>& from, const std::vector<seg_s>& to,
                const std::vector<int32_t>& gs, const std::vector<int32_t>& gd,
                const std::vector<xsbox>& boxes, uint64_t bytes);
    int execute(void* const* src, int ns, void* const* dst, int nd, void* stream) const;
};

// unstructured fused plan
struct uplan
{
    int direction = 0;
    uint64_t bytes = 0;
    int32_t n_segments = 0;
    uint32_t tile_bytes = kTileBytes;
    int max_field_slot = -1, max_buf_slot = -1;
    std::vector<launch_group<seg_u>> groups;  // host_segs: the launch-time choice of the run path
    device_tables lid_store;                  // lids: the index lists of every group's segments
    parity_cfg parity;
    bool grouped() const { return ghx::grouped(groups); }
    uint32_t total_tiles() const { return ghx::total_tiles(groups); }
    uplan(const ghx_upack_entry* entries, int n_entries, int direction);
    int execute(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;
};

// Index-list put (k_put_u): message k's send list on the sending field and its
// receive list on the receiving field, planned together: one row decomposition per message
// (uplan's rule applied to both sides), tiles by the index-list rule, one tile record per
// workgroup. Field slots: the sender's index the source pointer array, the receiver's the
// target pointer array; fewer than GHX_MAX_SLOTS of each (one launch). Built without a device;
// the records are kept on the host for inspection and uploaded when there is a device.
//
// The fused index-list self exchange (k_self_u, make_uself) is the same plan with a buffer side:
// `buf[k]` places message k in a send buffer, the segments carry their buffer slot and offset
// (which narrows wlog2 like any other offset), and both sides' field slots index ONE pointer
// array. execute_self stores every value to the buffer and to the target field in one launch.
struct ubuf_place
{
    int32_t slot;
    uint64_t off;
};
struct uput_plan
{
    uint64_t bytes = 0;            // message bytes moved per execution
    int max_src_slot = -1, max_dst_slot = -1;
    int max_buf_slot = -1;         // -1: a put (no buffer side)
    std::vector<seg_up> segs;      // plan order, first_tile 0
    std::vector<int32_t> message;  // per segment: its message, and
    std::vector<int64_t> first;    // its first position in that message's lists
    std::vector<seg_up> recs;      // one per tile, dispatch order
    bool run_ok = false;           // every segment may take the run path (urun on, mode 0, rows
                                   // of 4 or 8 B, tiles of whole 16-B chunks)
    device_tables dev;             // recs: the tile records; lids: both sides' index lists
    uput_plan(const ghx_uput_entry* src, const ghx_uput_entry* dst, int n,
              const ubuf_place* buf = nullptr);
    int execute(void* const* src, int ns, void* const* dst, int nd, void* stream) const;
    // The mixed form (make_umixed, k_pack_self_u): the pack plan of the messages that leave the
    // rank, one launch group with the caller's slots, and its tile records in dispatch order
    // (kept whatever g_tune.tile_records says). The launch runs them after the self tiles.
    std::unique_ptr<uplan> peers;
    std::vector<seg_u> peer_recs;
    device_tables peer_dev;        // recs: peer_recs
    // a plan with a buffer side: fields (both sides' slots) and send buffers, ONE launch
    int execute_self(void* const* fptr, int nf, void* const* bptr, int nb, void* stream) const;
};
// The plan of ghx_uself_create: src[k] / dst[k] are the pack and the unpack entry of the same
// message bytes. Throws `invalid` with the reason for what one fused launch cannot serve or would
// not do exactly as pack followed by unpack does (see include/ghx.h).
std::unique_ptr<uput_plan> make_uself(const ghx_upack_entry* src, const ghx_upack_entry* dst, int n);
// The plan of ghx_umixed_create: make_uself's plan of the self messages with the pack plan of
// `peers` (the plan a uplan of direction 0 makes of them) for the same launch. Refuses, beyond
// make_uself's reasons, a peer message that shares buffer bytes with another message and a peer
// source cell that a self message writes: the launch then equals pack followed by unpack.
std::unique_ptr<uput_plan> make_umixed(const ghx_upack_entry* src, const ghx_upack_entry* dst, int n_self,
                                       const ghx_upack_entry* peers, int n_peers);

// Adjoint accumulate (k_accum_u, ghx_accum_plan.cpp): the inverted index of the
// contribution entries (see include/ghx.h, ghx_uaccum_create). Destinations [0, n_dest) are the
// sum destinations, sorted by (field slot, lid), the next n_zero_dest the zero destinations,
// sorted alike; tiles [0, n_sum_tiles) cover the former, the rest the latter, so a launch without
// zero_halos runs the first n_sum_tiles only. Built without a device; the tables are kept on the
// host for inspection and uploaded when there is a device.
struct uaccum_plan
{
    uint64_t bytes = 0;                 // buffer bytes read per execution
    uint64_t n_dest = 0, n_zero_dest = 0;
    uint32_t max_per_dest = 0;
    uint32_t n_sum_tiles = 0;
    bool lid64 = false;
    int max_field_slot = -1, max_buf_slot = -1;  // of both kinds of entries
    std::vector<int32_t> dest_slot;     // per destination
    std::vector<int64_t> dest_lid;
    std::vector<acc_range> ranges;      // per sum destination
    std::vector<acc_contrib> contribs;  // by destination, then (entry, position)
    std::vector<acc_entry> entries;     // per contribution entry
    std::vector<uint8_t> entry_elem;    // and its element size
    std::vector<acc_tile> tiles;
    uint8_t slot_elem[GHX_MAX_SLOTS] = {};  // element size per field slot (0: slot unused)
    struct tables
    {
        void *tiles = nullptr, *ranges = nullptr, *lids = nullptr, *contribs = nullptr, *entries = nullptr;
        tables() = default;
        tables(const tables&) = delete;
        tables& operator=(const tables&) = delete;
        ~tables();
    } dev;
    // A get plan (ghx_uaccum_get_create, k_accum_get_u): `source` names per contribution entry the
    // halo side of the same message (null: the entry reads its buffer); position i of the entry's
    // list pairs with position i of the source's. The destinations, ranges, records and sum tiles
    // are those of the plain plan; src_lid holds per record the source lid (-1: a buffer record)
    // and get_entries per entry where its values lie. A zero entry that is a contribution's source
    // (same field slot, same list) gets no zero tile: the accumulate zeroes it as it reads.
    // rec64: a source lid is 2^31 or more and the device records are acc_get_rec64.
    bool get = false, rec64 = false;
    uint64_t n_field_sources = 0;       // contribution entries with a source
    std::vector<int64_t> src_lid;
    std::vector<acc_get_entry> get_entries;
    uaccum_plan(const ghx_upack_entry* contrib, const int32_t* dtypes, int n, const ghx_upack_entry* zero,
                int n_zero, const ghx_upack_entry* const* source = nullptr);
    int execute(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const;
    // a get plan's launch (ghx_uaccum_get_execute); each of the two refuses the other kind of plan
    int execute_get(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const;
};

// Adjoint accumulate of structured fields (k_accum_s, ghx_saccum_plan.cpp): the
// arrangement of the contribution boxes (see include/ghx.h, ghx_saccum_create). Sub-boxes
// [0, n_sum_boxes) are the sum sub-boxes, by field slot, the rest the zero entries' boxes; tiles
// [0, n_sum_tiles) cover the former, so a launch without zero_halos runs those only. Built without
// a device; the tables are kept on the host for inspection and uploaded when there is a device.
struct saccum_box
{
    int32_t field_slot;
    bool zero;
    int32_t first[GHX_MAX_DIM], last[GHX_MAX_DIM];  // spatial dims, the field's local coordinates
    uint64_t row_elems;
    uint8_t wlog2;
    uint32_t first_src, n_src;
};
struct saccum_plan
{
    uint64_t bytes = 0;                  // buffer bytes read per execution
    uint32_t n_sum_boxes = 0, n_sum_tiles = 0, max_sources = 0;
    int max_field_slot = -1, max_buf_slot = -1;  // of both kinds of entries
    std::vector<saccum_box> boxes;
    std::vector<sacc_src> srcs;          // by sub-box, each list in ascending (entry, box)
    std::vector<uint32_t> src_entry, src_box;  // per source record: the contribution box it is
    std::vector<sacc_tile> tiles;
    uint8_t slot_elem[GHX_MAX_SLOTS] = {};  // element size per field slot (0: slot unused)
    uint8_t buf_elem[GHX_MAX_SLOTS] = {};   // per buffer slot (0: slot unused)
    struct tables
    {
        void *tiles = nullptr, *srcs = nullptr;
        tables() = default;
        tables(const tables&) = delete;
        tables& operator=(const tables&) = delete;
        ~tables();
    } dev;
    // A get plan (ghx_saccum_get_create, k_accum_get_s): `source` names per contribution entry the
    // halo side of the same message (null: the entry reads its buffer). Source records then index
    // the table tab_slot: first the buffer slots that are read, ascending, then the source field
    // slots, ascending (tab_field: from where on). A zero entry that is a contribution's source
    // (same field slot, same boxes) gets no zero tile: the accumulate zeroes it as it reads.
    bool get = false;
    std::vector<int32_t> tab_slot;
    uint32_t tab_field = 0, n_field_sources = 0;
    // A cubed-sphere get plan (ghx_cs_exchange_adjoint_self_create, k_accum_get_x): `space` gives per
    // contribution entry with a source the receiving side of each of its boxes as cs_space_box
    // describes it (axes of the dense box in layout order). A paired box then reads the halo cell
    // its cell is the image of: origin and signed strides from the space, and the components the
    // edge negates in the source record's flags. n_rotated_sources: the paired boxes whose source
    // is not addressed as the receiving field's own box would be (transposed, reversed or signed).
    bool rotated = false;
    uint32_t n_rotated_sources = 0;
    struct source_map  // per source record, for inspection: its signed byte stride per dimension of
    {                  // the contribution's field, the components it negates, the component dimension
        int64_t stride[GHX_MAX_DIM];
        uint8_t neg;
        int8_t comp_dim;
    };
    std::vector<source_map> src_map;
    saccum_plan(const ghx_pack_entry* contrib, const int32_t* dtypes, int n, const ghx_pack_entry* zero,
                int n_zero, const ghx_pack_entry* const* source = nullptr, const xseg* const* space = nullptr);
    int execute(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const;
    // a get plan's launch (ghx_saccum_get_execute); each of the two refuses the other kind of plan
    int execute_get(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const;

private:
    int launch(void* const* fptr, int nf, void* const* bptr, int nb, bool zero_halos, void* stream) const;
};

// The per-call entry points' plans, cached by content (ghx_cache.cpp): the plan of the call's
// descriptor and spaces, or index list, is built on first use and executed on `stream`.
int run_structured(const ghx_field_desc& f, const ghx_box* boxes, int n, int dir, void* field,
                   void* buffer, void* stream);
int run_cs_unpack(const ghx_field_desc& f, const ghx_cs_item& cs, const ghx_box* local,
                  const ghx_box* global, const int32_t* tiles, int n, void* field, void* buffer,
                  void* stream);
// the transpose of run_cs_unpack (ghx_cs_pack_rotated): the same cached plan, field -> buffer
int run_cs_pack_rotated(const ghx_field_desc& f, const ghx_cs_item& cs, const ghx_box* local,
                        const ghx_box* global, const int32_t* tiles, int n, const void* field,
                        void* buffer, void* stream);
int run_unstructured(const ghx_udata_desc& d, const void* lids, int32_t lid_bytes, int64_t n,
                     int dir, void* values, void* buffer, void* stream);
}  // namespace ghx

// opaque handles
struct ghx_plan : ghx::splan
{
    using ghx::splan::splan;
};
struct ghx_uplan : ghx::uplan
{
    using ghx::uplan::uplan;
};
struct ghx_uaccum : ghx::uaccum_plan
{
    using ghx::uaccum_plan::uaccum_plan;
};
struct ghx_saccum : ghx::saccum_plan
{
    using ghx::saccum_plan::saccum_plan;
};
