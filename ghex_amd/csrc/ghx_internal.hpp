// ghx_internal.hpp — structures shared by the host planner and the gfx950 kernels.
//
// Data layout in HBM: a plan is a flat table of segments (one per field x
// iteration space) plus a tile table (uint32 segment index per workgroup tile). A segment is a
// set of equal-length contiguous byte runs ("rows") of the field that map, in order, onto ONE
// contiguous byte range of the buffer — the dense buffer box of make_buffer_desc
// (include/ghex/structured/regular/field_descriptor.hpp:114-129) is row-major in the field's
// layout order, so row r occupies buffer bytes [r*L, (r+1)*L). Rows are decoded from the
// buffer byte position by magic-number division (no hardware divide on the hot path).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghx.h"

namespace ghx
{
// Bytes of buffer covered by one workgroup tile (default 256 threads x 4 vectors x 16 B); the
// tile size is a plan-time tuning knob bounded by kMaxTileBytes.
constexpr uint32_t kTileBytes = 8192;
constexpr uint32_t kMaxTileBytes = 1u << 20;
constexpr int kBlock = 256;

// Launch / planning knobs (ghx_tune). Defaults are the measured best. The knobs
// whose every setting but the default lost its A/B were removed in round 3
// (tools/kernel_variants_r02.hip lists them with their numbers).
struct tuning
{
    int grid_cap = 0;               // >0: at most this many workgroups (grid-stride beyond)
    uint32_t tile_bytes = kTileBytes;  // tile of segments with long rows
    uint32_t unpack_tile_bytes = 0;    // the same for unpack plans (0: tile_bytes); above 8 KiB
                                       // the unpack kernel pipelines a tile's steps
    uint32_t self_tile_bytes = kTileBytes;  // the same for the fused self exchange (separate
                                       // self plans are built when it differs). Medians of 4
                                       // interleaved A/B runs with register forwarding:
                                       // H=2 8 KiB 26.4 vs 4 KiB 27.9 us; H=1 18.6 vs 19.9;
                                       // H=3 32.8 vs 32.0 (profiles/r01c_fwd_tile_ab.jsonl)
    uint32_t small_tile_rows = 0;      // rows per tile of segments with short rows (0: by the
                                       // plan's short-row count, ghx_plan.cpp short_tile_rows)
    uint32_t pack_tile_rows = 0;       // rows per short-row tile of PACK plans only (0: as
                                       // small_tile_rows / the plan's rule)
    uint32_t unpack_tile_rows = 0;     // the same for UNPACK plans
    uint32_t small_row_bytes = 64;     // rows shorter than this are "short" (request-bound)
    uint32_t u_tile_rows = 512;        // rows per tile of short-row unstructured segments
    uint32_t u_tile_bytes = 16384;     // tile of unstructured segments with long rows (config 5's
                                       // 64-B levels-first rows: scatter 16.8 -> 14.0 us against
                                       // 8 KiB, tools/u_tile_sweep.py, profiles/r05_u_tile_sweep*)
    int order = 1;                     // tile dispatch order: 0 segment order, 1 short-row
                                       // segments first (2-4 lost: tools/kernel_variants_r02.hip)
    int urun = 1;                      // unstructured 4/8-B-row segments: 16-B lane chunks with
                                       // run detection (copy_runs)
    uint32_t u_run_tile_rows = 2048;   // rows per tile of run-heavy index-list segments
    int short_pol = 0;                 // field-side cache policy of short-row segments:
                                       // bit 0 non-temporal loads (pack), bit 1 sc1 stores
                                       // (unpack)
    int xcd_pair = 1;                  // dispatch the tiles of line-sharing short-row segment
                                       // pairs in lock-step groups of 8, so tile t of both
                                       // halves lands on the same XCD (blocks are dealt
                                       // round-robin over the 8 XCDs) at the same time
    int mixed_always = 0;              // build the mixed self/peer plans even when the self
                                       // messages hold no short rows (tests, measurements)
    int tile_records = 1;              // k_copy reads per tile ONE record (its segment with the
                                       // tile index in first_tile) at blockIdx: no dependent
                                       // tile-table load ahead of the segment load
    uint32_t x_tile_elems = 256;       // elements per tile of transformed (cubed-sphere)
                                       // segments: one per lane (512 and 1024
                                       // lost to the element-row form, 128 ties 256)
    int fast_addr = 1;                 // structured segments whose offsets fit the short form
                                       // (seg_s::amode) decode rows with 1-2 divisions and
                                       // full-rate 24-bit products instead of int64 ones
};
extern tuning g_tune;

// Unsigned 32-bit division by an invariant d via multiply-high (Granlund-Montgomery; the
// round-up variant valid for every n < 2^32): q = (t + ((n - t) >> s1)) >> s2, t = mulhi(m, n).
struct magic_u32
{
    uint32_t m;
    uint8_t s1, s2;
    uint16_t pad;
};

inline magic_u32 make_magic(uint32_t d)
{
    magic_u32 r{};
    if (d == 0) d = 1;
    int l = 0;
    while ((uint64_t(1) << l) < d) ++l;  // l = ceil(log2 d)
    uint64_t m = ((uint64_t(1) << 32) * ((uint64_t(1) << l) - d)) / d + 1;
    r.m = uint32_t(m);
    r.s1 = uint8_t(l < 1 ? l : 1);
    r.s2 = uint8_t(l > 1 ? l - 1 : 0);
    return r;
}

// Structured segment (128 B, read once per workgroup tile with scalar loads).
struct alignas(16) seg_s
{
    int64_t field_off;    // byte offset (from the field base) of the segment's first row
    uint64_t buf_off;     // byte offset (from the buffer base) of the segment's first byte
    int64_t stride[4];    // field byte stride of outer dim k (k = 0 varies fastest over rows)
    uint32_t ext[4];      // outer extents (1 for unused dims)
    magic_u32 mag_row;    // division by row_bytes
    magic_u32 mag_ext[3]; // division by ext[0], ext[1], ext[2]
    uint32_t row_bytes;   // L: bytes per contiguous run
    uint32_t bytes;       // rows * L
    uint32_t first_tile;  // 0 in a segment table; in a tile record, the tile's index in its
                          // segment
    uint16_t field_slot;
    uint16_t buf_slot;
    uint8_t wlog2;        // log2 of the widest vector (<= 16 B) that divides L, offsets, strides
    uint8_t n_outer;
    uint8_t fpol;         // field-side cache policy: bit 0 nt loads, bit 1 sc1 stores
    uint8_t pipe;         // unpack of long rows in tiles of several steps: software-pipelined
    uint32_t tile_bytes;  // this segment's tile size (a multiple of the row length or 16 KiB)
    uint8_t amode;        // field-offset arithmetic (planner, set_amode): 0 general (int64, 3
                          // divisions), 1 / 2: 32-bit offsets relative to field_off from 24-bit
                          // products, 1 / 2 divisions (n_outer <= 2 / == 3), see field_offset_f
    uint8_t pad[7];
};
static_assert(sizeof(seg_s) == 128, "seg_s layout");

// Unstructured segment: rows come from an index list.
struct alignas(16) seg_u
{
    uint64_t buf_off;
    const void* lids;          // device array, int32 or int64
    int64_t index_stride_b;    // bytes
    int64_t level_stride_b;    // bytes
    magic_u32 mag_row;         // division by row_bytes
    magic_u32 mag_inner;       // levels_first: division by levels_per_row-group; else by n
    uint32_t n;                // number of indices
    uint32_t row_levels;       // levels per row group when rows are per (i,l); see planner
    uint32_t row_bytes;
    uint32_t bytes;
    uint32_t first_tile;
    uint16_t field_slot;
    uint16_t buf_slot;
    uint8_t wlog2;
    uint8_t mode;              // 0: row = index i (levels contiguous, L = levels*elem)
                               // 1: rows (i,l) i-major (levels_first, strided levels)
                               // 2: rows (l,i) l-major (levels_last)
    uint8_t lid64;
    uint8_t fpol;              // field-side cache policy (as seg_s)
    uint32_t tile_bytes;
    int64_t field_off;         // added to every field offset (a level of a split levels-last list)
    uint8_t runs;              // mode 0, rows of 4 or 8 B, rows of consecutive lids contiguous
                               // in the field: lanes move 16-B chunks (16/L rows), one 16-B
                               // field access where the chunk's lids form a run (copy_runs);
                               // 2: at least half the chunks are runs (u_run_tile_rows tiles)
    uint8_t pad2[7];
};
static_assert(sizeof(seg_u) == 96, "seg_u layout");

// Index-list put segment (k_put_u): the send list of a message on the sending
// field and the receive list of the same message on the receiving field, with ONE row
// decomposition of the message bytes for both sides (mode, row_bytes, mag_*: as seg_u's). Message
// row r = (i, l) by `mode` sits at field_off + lid[i] * index_stride_b + l * level_stride_b of
// its side. A put has no buffer; its tile records are this record with the tile's index in
// first_tile, one per workgroup. The fused self exchange (k_self_u) uses the same record with the
// message's place in its send buffer: message row r at buf_off + r * row_bytes of buffer buf_slot
// in every mode (a put leaves both zero and never reads them).
struct alignas(16) seg_up
{
    const void* src_lids;      // device arrays, int32 or int64 per side
    const void* dst_lids;
    int64_t src_index_stride_b, src_level_stride_b, src_field_off;
    int64_t dst_index_stride_b, dst_level_stride_b, dst_field_off;
    magic_u32 mag_row;         // division by row_bytes
    magic_u32 mag_inner;       // mode 1: by the levels; mode 2: by n
    uint32_t n;                // number of indices
    uint32_t row_levels;       // mode 1: the levels
    uint32_t row_bytes;
    uint32_t bytes;
    uint32_t first_tile;
    uint32_t tile_bytes;
    uint16_t src_slot, dst_slot;
    uint8_t wlog2;             // widest vector dividing the row and both sides' offsets and strides
                               // (and buf_off, in a self exchange)
    uint8_t mode;              // as seg_u::mode, common to both sides
    uint8_t src_lid64, dst_lid64;
    uint8_t src_runs, dst_runs;  // the side's rows of consecutive lids are adjacent (4/8-B rows,
                                 // mode 0, index stride = row): it may move a 16-B chunk in one
                                 // access (put_runs); 2: at least half of its chunks are runs
    uint16_t buf_slot;         // self exchange: the send buffer of the message, and
    uint8_t pad[4];
    uint64_t buf_off;          // the byte offset of the segment's first row in it
};
static_assert(sizeof(seg_up) == 128, "seg_up layout");

// Transformed segment (cubed sphere): an iteration space received from another
// cube tile whose rotation moves or reverses the field's stride-1 axis, or negates a vector
// component (cubed_sphere/field_descriptor.hpp:81-108). The buffer holds the dense box in the
// NEIGHBOUR's coordinates, row-major in the field's layout order; each buffer axis has a signed
// field byte stride. `xseg` is the planner's description of the whole box (axes in buffer order,
// 0 = fastest); `seg_x` is the record of ONE workgroup tile of it (k_unpack_x reads the record at
// its block index): a sub-box of about one element per lane that is wide along BOTH the
// buffer's fastest axis and the field's, walked with its axes sorted by ascending |field
// stride| — a wave reads a few long buffer row pieces and writes whole field runs, so neither
// side is walked element by element across lines.
struct xseg
{
    int64_t field_off;   // field byte offset of buffer cell (0, 0, 0, 0)
    uint64_t buf_off;    // byte offset of the box in its buffer
    int64_t stride[4];   // signed field byte stride per buffer axis
    uint32_t ext[4];     // extents in buffer order (1 for unused axes)
    uint32_t elem;       // 1, 2, 4, 8 or 16 bytes
    int32_t comp_axis;   // the buffer axis that is the component axis (-1: none)
    uint8_t neg_mask;    // bit k: component k is negated (k = 0, 1)
    uint8_t neg_kind;    // 1: IEEE sign-bit flip, 2: two's-complement negate
    int32_t field_slot, buf_slot;  // the caller's slots
    uint32_t tile_elems; // the planner's tile size in elements
    uint64_t bytes() const { return uint64_t(ext[0]) * ext[1] * ext[2] * ext[3] * elem; }
};

struct alignas(16) seg_x
{
    int64_t field_off;    // field byte offset of the tile's first cell
    uint64_t buf_off;     // byte offset of the tile's first cell in its buffer
    int64_t stride[4];    // field byte stride per tile axis; axes by ascending |stride|
    uint32_t tdim[4];     // the plan's tile extents per axis (decode radix)
    uint32_t act[4];      // this tile's extents (<= tdim: the last tile along an axis)
    uint32_t bstride[4];  // element stride of the axis in the buffer's dense box
    magic_u32 mag[4];     // division by tdim[k]
    uint32_t bytes;       // bytes this tile moves
    uint32_t comp0;       // component index of the tile's first cell
    uint16_t field_slot;
    uint16_t buf_slot;
    uint8_t elog2;        // log2 of the element size
    uint8_t comp_pos;     // which of the four axes is the component axis (4: none)
    uint8_t neg_mask;
    uint8_t neg_kind;
};
static_assert(sizeof(seg_x) == 144, "seg_x layout");

// Self tile record (fused cubed-sphere self exchange): a seg_x tile of the
// RECEIVING field plus the SENDING side of the same buffer cells. The buffer box is the sender's
// dense box in the sender's own coordinates, so the source address is affine in the tile
// coordinates as the destination's is: src_off + sum c_k * src_stride[k], the axes those of `x`.
// k_self_cs loads the element from the source field, stores it unmodified to the buffer cell and,
// negated as `x` says, to the destination field.
struct alignas(16) seg_xs
{
    seg_x x;                // destination tile (x.field_slot, x.field_off, x.stride) and buffer side
    int64_t src_off;        // source field byte offset of the tile's first cell
    int64_t src_stride[4];  // signed source field byte stride per tile axis
    uint16_t src_slot;      // field slot of the sending field
    uint8_t pad[6];
};
static_assert(sizeof(seg_xs) == 192, "seg_xs layout");
static_assert(alignof(seg_xs) == 16, "seg_xs alignment");

// Kernel arguments (passed by value: <= 1.7 KB of kernarg).
struct kargs
{
    const void* segs;
    const void* segs2;         // fused self exchange: the unpack segments (1:1 with segs)
    const uint32_t* tile_seg;  // per tile: {segment index, tile index within the segment}
    const void* tile_recs;     // or per tile one record (k_copy; null: use segs + tile_seg)
    uint32_t n_tiles;
    uint32_t parity_add;       // double-buffered launches: parity = (*parity_word + add) & 1
    const uint64_t* parity_word;  // null: single-buffered (the kernels' plain variants)
    uint64_t field_ptr[GHX_MAX_SLOTS];
    uint64_t buf_ptr[GHX_MAX_SLOTS];
    int64_t dbl_off[GHX_MAX_SLOTS];  // per buffer slot: byte offset of its odd-parity copy (0: none)
};

// Arguments of the fused cubed-sphere self exchange (k_self_cs): blocks [0, n_pair_tiles) take
// the pair record (two seg_s, as k_self's) at their index, the next n_x_tiles a seg_xs record.
// One pointer array holds the field pointers (slot s at ptr[s]) and after them the buffer
// pointers (slot b at ptr[buf_base + b]): a whole cube on one rank has few fields and many
// domain-pair buffers (24 domains: 168), more than kargs' GHX_MAX_SLOTS of each, and the launch
// is only worth having if it is ONE launch. 3.6 KB of kernarg.
constexpr int kCsSelfPtrs = 448;
struct kargs_cs
{
    const void* pair_recs;
    const void* x_recs;
    uint32_t n_pair_tiles;
    uint32_t n_x_tiles;
    uint32_t buf_base;
    uint32_t pad;
    uint64_t ptr[kCsSelfPtrs];
};
static_assert(sizeof(kargs_cs) < 4096, "kargs_cs is passed by value");

// Arguments of the cubed-sphere put (k_put_cs): blocks [0, n_pair_tiles) take the pair record
// (two seg_s, as k_put's record form) at their index, the next n_x_tiles a put tile record
// (seg_xs, buffer side unused). Source field slot s at src_ptr[s], target field slot d at
// dst_ptr[d], as k_put's field_ptr / buf_ptr.
struct kargs_pcs
{
    const void* pair_recs;
    const void* x_recs;
    uint32_t n_pair_tiles;
    uint32_t n_x_tiles;
    uint64_t src_ptr[GHX_MAX_SLOTS];
    uint64_t dst_ptr[GHX_MAX_SLOTS];
};

// Arguments of the index-list pack that also completes the self messages (k_pack_self_u): blocks
// [0, n_self_tiles) take the seg_up record (with its buffer side, as k_self_u's) at their index,
// the next n_peer_tiles a seg_u tile record of the peer messages' pack plan. Field slots of both
// parts index field_ptr, buffer slots the send buffers in buf_ptr.
struct kargs_um
{
    const void* self_recs;
    const void* peer_recs;
    uint32_t n_self_tiles;
    uint32_t n_peer_tiles;
    uint64_t field_ptr[GHX_MAX_SLOTS];
    uint64_t buf_ptr[GHX_MAX_SLOTS];
};

// Adjoint accumulate (k_accum_u, ghx_accum.hip): the tables of a uaccum_plan.
// Destination d (a cell of a field; sum destinations first, sorted by field slot then lid, then
// the zero destinations, sorted alike) has its lid in the plan's lid table and, a sum
// destination, its range [first, first + count) of the contribution records in acc_range.
// A contribution record names (entry, position in that entry's list); records of one destination
// ascend by (entry, position), which is the order of the adds. The entry record turns (position,
// level) into a buffer address: element position * pos_stride + level * lev_stride from buf_off
// on (levels_first: [i][level], strides (levels, 1); else [level][i], strides (1, n)).
struct acc_range
{
    uint32_t first, count;
};
struct acc_contrib
{
    uint32_t entry, pos;
};
struct alignas(16) acc_entry
{
    uint64_t buf_off;      // bytes, a multiple of the element size
    uint32_t n;
    uint32_t levels;
    uint32_t levels_first;
    uint32_t buf_slot;
    uint32_t pos_stride;   // in elements
    uint32_t lev_stride;
};
static_assert(sizeof(acc_entry) == 32, "acc_entry layout");
// Tile record, one per workgroup tile: n_rows destinations from first_dest on, all of one field
// slot (whose descriptor every entry of the slot shares). A lane takes element (row r, level l) of
// the tile's n_rows * levels: lcontig (levels adjacent in the field) r = e / levels, else
// l = e / n_rows, `mag` dividing by that. zero: store zero bytes, read nothing.
struct alignas(16) acc_tile
{
    int64_t index_stride_b;
    int64_t level_stride_b;
    uint32_t first_dest;
    uint32_t n_rows;
    uint32_t levels;
    magic_u32 mag;
    uint16_t field_slot;
    uint8_t dtype;         // GHX_DT_* (a zero tile: any dtype of the slot's element size)
    uint8_t zero;
    uint8_t lcontig;
    uint8_t pad[7];
};
static_assert(sizeof(acc_tile) == 48, "acc_tile layout");
struct kargs_ua
{
    const acc_tile* tiles;
    const acc_range* ranges;
    const void* lids;          // per destination, int32 or int64 (lid64)
    const acc_contrib* contribs;
    const acc_entry* entries;
    uint32_t n_tiles;
    uint32_t lid64;
    uint64_t field_ptr[GHX_MAX_SLOTS];
    uint64_t buf_ptr[GHX_MAX_SLOTS];
};

// The get form (k_accum_get_u, ghx_uaccum_get_create): the destination, range and tile tables of
// above; what changes is where a record's value is loaded from. A record names its entry and an
// index `at`: the position in the message for an entry that reads its buffer, the SOURCE LID for
// an entry that reads the halo cells of a receiving field (resolved by the planner, so a lane's
// chain is record -> entry -> value for both). Records are acc_get_rec, or acc_get_rec64 when a
// source lid is 2^31 or more (one table per plan, kargs_uag::rec64). The entry record gives the
// element strides of `at` and of the level and the pointer the value lies behind: the value of
// (at, level) is at ptr[tab] + base + (at * at_stride + level * lev_stride) * sizeof(T).
struct acc_get_rec
{
    uint32_t entry, at;
};
struct alignas(16) acc_get_rec64
{
    uint32_t entry, pad;
    uint64_t at;
};
struct alignas(16) acc_get_entry
{
    uint64_t base;        // buffer: the message's byte offset; field source: 0
    int64_t at_stride;    // in elements. Buffer: 1 or levels; field source: its index stride
    int64_t lev_stride;   // buffer: n or 1; field source: its level stride
    uint32_t tab;         // index in kargs_uag::ptr
    uint32_t field_src;   // 1: a field source, which the loading lane zeroes in a launch with zero_src
};
static_assert(sizeof(acc_get_entry) == 32, "acc_get_entry layout");
struct kargs_uag
{
    const acc_tile* tiles;
    const acc_range* ranges;
    const void* lids;          // per destination, int32 or int64 (lid64)
    const void* recs;          // acc_get_rec or acc_get_rec64 (rec64)
    const acc_get_entry* entries;
    uint32_t n_tiles;
    uint32_t lid64;
    uint32_t rec64;
    uint32_t zero_src;         // store zero over a field source once it is loaded (zero_halos)
    // field slot s at [s] (owners and sources alike), buffer slot b at [GHX_MAX_SLOTS + b]
    uint64_t ptr[2 * GHX_MAX_SLOTS];
};

// Adjoint accumulate of structured fields (k_accum_s, ghx_accum.hip): the tables
// of a saccum_plan. The union of a field's contribution boxes is cut into disjoint sub-boxes; every
// cell of a sub-box has the same sources — the contribution boxes that hold it, in ascending
// (entry, box) — so the source list belongs to the sub-box and is uniform over a workgroup.
// A sub-box is a set of equal rows (runs along the layout's fastest dimension; one element each
// where that dimension is strided in the field) decoded from the row index as seg_s's rows are:
// outer coordinate c_k = (row / (ext[0] .. ext[k-1])) % ext[k], row at field_off + sum c_k *
// stride[k]. A row is a contiguous piece of one buffer row of each source: the source record holds
// the buffer offset of the sub-box's origin in that box's dense buffer box and the box's buffer
// byte strides for the same outer coordinates.
struct alignas(16) sacc_src
{
    uint64_t buf_off;     // byte offset in the buffer of the sub-box's origin
    uint64_t stride[4];   // buffer byte stride of outer dim k of the sub-box in this box
    uint32_t buf_slot;    // index in the launch's source pointer table (kargs_sa::buf_ptr)
    uint32_t flags;       // bit 0: a field source (k_accum_get_s: a receiving field's halo cells,
                          // zeroed after the load when the launch has zero_halos); bits 1-2: the
                          // vector components 0 / 1 this source negates (k_accum_get_x: a halo read
                          // across a cube edge, strides signed mod 2^64); else 0
};
static_assert(sizeof(sacc_src) == 48, "sacc_src layout");
constexpr uint32_t kSaccFieldSrc = 1u;
constexpr uint32_t kSaccNegShift = 1;
// sacc_tile::comp: where the component index of a lane's vector comes from
constexpr uint8_t kSaccCompNone = 0;  // no source of the sub-box negates some components and not others
constexpr uint8_t kSaccCompRow = 5;   // the row is one vector of the field: byte column / element size
                                      // (1..4: outer coordinate c[comp - 1])
// Tile record, one per workgroup tile: the sub-box with the tile's part of it — n_rows rows from
// first_row on, of each the `len` bytes from byte col0 on (col0 > 0 only where one row is longer
// than a tile: then n_rows = 1 and col0 a multiple of 16). A lane takes one vector of the tile's
// n_rows * len bytes, rows outermost. zero: store zero bytes, read nothing (no sources).
struct alignas(16) sacc_tile
{
    int64_t field_off;    // field byte offset of the sub-box's origin
    int64_t stride[4];    // field byte stride of outer dim k (k = 0 varies fastest over rows)
    uint64_t buf_mask;    // bit b: a source of the sub-box reads buffer slot b
    uint32_t ext[4];      // outer extents (1 for unused dims)
    magic_u32 mag_ext[3]; // division by ext[0], ext[1], ext[2]
    magic_u32 mag_vec;    // division by len >> wlog2, the planned vectors of a row piece
    uint32_t len;         // bytes of a row this tile covers (the row length unless col0 / cut)
    uint32_t col0;
    uint32_t first_row;
    uint32_t n_rows;
    uint32_t first_src;   // the sub-box's records [first_src, first_src + n_src) of sacc_src
    uint32_t n_src;
    uint16_t field_slot;
    uint8_t dtype;        // GHX_DT_* (a zero tile: any dtype of the slot's element size)
    uint8_t zero;
    uint8_t wlog2;        // log2 of the widest vector (<= 16 B) dividing the row, the field offset
                          // and strides and every source's buffer offset and strides
    uint8_t n_outer;
    uint8_t comp;         // k_accum_get_x: kSaccComp*, which tile axis carries the components a
                          // source's mask (sacc_src::flags) speaks of; 0 in every other plan
    uint8_t pad;
};
static_assert(sizeof(sacc_tile) == 128, "sacc_tile layout");
struct kargs_sa
{
    const sacc_tile* tiles;
    const sacc_src* srcs;
    uint32_t n_tiles;
    uint32_t zero_src;             // k_accum_get_s: store zero bytes over a field source once loaded
    uint64_t buf_mis8, buf_mis16;  // bit b: source pointer b is not 8- / 16-byte aligned
    uint64_t field_ptr[GHX_MAX_SLOTS];
    // the source pointer table: the buffers; in a get plan the buffers that are read, then the
    // source fields (saccum_plan::tab_slot)
    uint64_t buf_ptr[GHX_MAX_SLOTS];
};

// Double-buffered buffers (the direct exchange's one-launch epochs, ghx_epochs.hip): a buffer
// exists twice, its odd-parity copy `offset` bytes after the even one, and a launch uses the copy
// of the exchange's parity, read on the device from the epoch counter (so that a captured graph
// alternates on replay). Per caller buffer index: the offset (0 = one copy only).
struct parity_cfg
{
    const uint64_t* word = nullptr;
    uint32_t add = 0;
    std::vector<int64_t> offset;
    // fill a launch's parity fields; map: local slot -> caller buffer index (empty: identity)
    void apply(kargs& a, const std::vector<int32_t>& map, int n_identity) const
    {
        if (!word) return;
        a.parity_word = word;
        a.parity_add = add;
        const int n = map.empty() ? n_identity : int(map.size());
        for (int i = 0; i < n; ++i)
        {
            const size_t c = size_t(map.empty() ? i : map[size_t(i)]);
            a.dbl_off[i] = c < offset.size() ? offset[c] : 0;
        }
    }
};

// thread-local last error
void set_error(const std::string& msg);
const char* get_error();

// kernel launchers (ghx_kernels.hip)
int launch_structured(const kargs& a, int direction, void* stream, uint32_t grid);
int launch_unstructured(const kargs& a, int direction, void* stream, uint32_t grid, bool runs);
int launch_self(const kargs& a, void* stream, uint32_t grid);
int launch_put(const kargs& a, void* stream, uint32_t grid);
int launch_unpack_x(const kargs& a, void* stream, uint32_t grid);  // tile_recs: seg_x records
int launch_pack_x(const kargs& a, void* stream, uint32_t grid);    // the same records, field -> buffer
int launch_self_cs(const kargs_cs& a, void* stream, uint32_t grid);
int launch_put_cs(const kargs_pcs& a, void* stream, uint32_t grid);
// tile_recs: seg_up records; field_ptr / buf_ptr: the source / target fields (as launch_put)
int launch_put_u(const kargs& a, void* stream, uint32_t grid, bool runs);
// tile_recs: seg_up records with their buffer side; field_ptr: the fields of both sides, buf_ptr:
// the send buffers
int launch_self_u(const kargs& a, void* stream, uint32_t grid, bool runs);
// self_recs: seg_up records with their buffer side, peer_recs: seg_u tile records (pack)
int launch_pack_self_u(const kargs_um& a, void* stream, uint32_t grid, bool runs);
// ghx_accum.hip: the adjoint accumulate over the first a.n_tiles tile records
int launch_accum_u(const kargs_ua& a, void* stream, uint32_t grid);
int launch_accum_get_u(const kargs_uag& a, void* stream, uint32_t grid);  // k_accum_get_u
int launch_accum_s(const kargs_sa& a, void* stream, uint32_t grid);
int launch_accum_get_s(const kargs_sa& a, void* stream, uint32_t grid);  // k_accum_get_s
int launch_accum_get_x(const kargs_sa& a, void* stream, uint32_t grid);  // k_accum_get_x
uint32_t grid_for_tiles(uint32_t n_tiles);
void timing_enable(bool on);                            // ghx_launch_timing
int timing_read(float* ms, int32_t cap, int32_t* n);    // ghx_launch_timing_read

}  // namespace ghx
