/*
 * ghx.h — C ABI of ghex_amd, the MI355X-native halo pack/unpack path for GHEX.
 *
 * Plain C: pointers, sizes and status codes only (no C++ or torch types cross this line).
 * The library is libghx.so (ghex_amd/lib/). Every entry point below names the reference
 * interface it replaces (paths relative to the GHEX v0.8.0 tree). INTEGRATION.md shows the
 * binding a GHEX maintainer would add on the reference side.
 *
 * Status: every function returns GHX_OK (0) or a negative ghx_status; ghx_last_error() then
 * returns a thread-local message. No exception crosses the ABI (the reference throws
 * std::runtime_error, include/ghex/device/cuda/error.hpp:21-25; the C++ adaptor in
 * include/ghex_amd/field_descriptor.hpp converts back to that convention).
 *
 * Threading: plans and patterns are immutable after creation; executing one plan from several
 * threads on distinct streams is safe. Executions are stream-ordered and asynchronous (no host
 * synchronisation inside ghx_*_execute / ghx_*_pack / ghx_*_unpack), so they can be captured
 * into a hipGraph.
 */
#ifndef GHX_H
#define GHX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ghx_status
{
    GHX_OK = 0,
    GHX_ERR_INVALID = -1,    /* bad argument (shape, layout, slot, alignment ...) */
    GHX_ERR_HIP = -2,        /* a HIP runtime call failed */
    GHX_ERR_NOMEM = -3,      /* host or device allocation failed */
    GHX_ERR_PATTERN = -4,    /* pattern construction failed (e.g. inconsistent halo gids) */
} ghx_status;

/* Opaque stream handle: a hipStream_t (NULL = the default stream). Kept as void* so that this
 * header needs no HIP include. Replaces the `void* arg` = cudaStream_t* of the reference's
 * field-descriptor concept (include/ghex/structured/pack_kernels.hpp:216-234). */
typedef void* ghx_stream;

#define GHX_MAX_DIM 4     /* 3 spatial dims + 1 component axis (bindings/python/src/_pyghex/structured/types.hpp:31-63) */
#define GHX_MAX_SLOTS 64  /* field / buffer pointer slots per kernel launch; a plan whose entries
                             use more is executed as one launch per group of <= 64 (any slot >= 0) */

/* Process-wide tuning knobs (development / benchmarking; defaults are the measured best):
 * "grid_cap" (max workgroups, 0 = one per tile), "tile_bytes" (buffer bytes per workgroup tile),
 * "small_tile_rows" (rows per tile of short-row structured segments; 0 = by the plan's count of
 * short rows, the default), "small_row_bytes" (rows
 * shorter than this are "short"), "order" (0 segment order, 1 short-row segments first),
 * "xcd_pair" (0|1: line-sharing short-row segment pairs dispatched in lock-step groups of 8
 * tiles, same XCD), "short_pol" (field-side cache policy of short-row segments: bit 0
 * non-temporal loads, bit 1 sc1 stores), "u_tile_rows" (rows per tile of short-row index-list
 * segments), "u_tile_bytes" (tile of index-list segments with long rows), "urun" (0|1: run path
 * for 4/8-B index-list rows), "u_run_tile_rows" (rows per tile of run-heavy index lists), "self_tile_bytes" (tile of the fused self exchange),
 * "mixed_always" (0|1: build mixed self/peer plans even without short-row self messages),
 * "tile_records" (0|1: the pack / unpack launches read one per-tile record addressed by the
 * workgroup index instead of a tile table entry and then its segment; default 1),
 * "unpack_tile_bytes" (0 = tile_bytes, the default; else the long-row tile of unpack plans, whose
 * tiles of several steps the unpack kernel then software-pipelines);
 * "fast_addr" (0|1: short-form 32-bit field addressing for segments whose extents, strides and
 * span fit it; default 1), "x_tile_elems" (elements per workgroup tile of the cubed-sphere
 * transformed unpack, 32..4096; default 256, one per lane), "pack_tile_rows" /
 * "unpack_tile_rows" (0 = by the plan's rule, the
 * default; else 64..65536 rows per tile of short-row structured segments of pack / unpack plans);
 * "reset" restores every default. Plan-shaping knobs apply to plans created afterwards. Unknown
 * keys fail with GHX_ERR_INVALID (the variants removed in round 3 are listed in
 * tools/kernel_variants_r02.hip).
 * No reference counterpart (the reference hard-codes block_dim=128, 1 element per thread:
 * include/ghex/structured/pack_kernels.hpp:211-214). */
int ghx_tune(const char* key, int32_t value);

/* Per-launch kernel durations (measurement; no reference counterpart). ghx_launch_timing(1) makes
 * every kernel launch issued afterwards BY THIS THREAD record a start and a stop event at the
 * kernel's own begin and end (hipExtLaunchKernel: the interval a rocprofv3 kernel trace reports);
 * eager launches only — never enable it around a stream capture. ghx_launch_timing_read waits for
 * the recorded launches, writes up to `cap` durations in milliseconds (launch order) to `ms`, the
 * number recorded to `*n`, and releases them; ghx_launch_timing(0) stops recording (and drops
 * unread records). */
int ghx_launch_timing(int32_t enable);
int ghx_launch_timing_read(float* ms, int32_t cap, int32_t* n);

/* Last error message of the calling thread ("" if none). */
const char* ghx_last_error(void);
/* Library version string and the offload target it was compiled for ("gfx950"). */
const char* ghx_version(void);

/* ------------------------------------------------------------------------------------------
 * Structured fields
 * ------------------------------------------------------------------------------------------ */

/* A wrapped structured field: the queries of the reference's field-descriptor concept
 * (doc_src/scope/scope.rst:331-359; include/ghex/structured/field_descriptor.hpp:27-41,
 * 152-226): dimension (incl. component axis), value size, layout_map, byte strides, offsets.
 * layout[d] = gridtools::layout_map<...>::at(d); the dim whose value is dim-1 is stride-1.
 * has_components: the last dim is the component axis of extent num_components (offset 0). */
typedef struct ghx_field_desc
{
    int32_t dim;
    int32_t elem_size;                 /* sizeof(value_type), any size >= 1 */
    int32_t layout[GHX_MAX_DIM];
    int64_t byte_strides[GHX_MAX_DIM];
    int32_t offsets[GHX_MAX_DIM];
    int32_t extents[GHX_MAX_DIM];      /* informational (bounds checks), incl. halos */
    int32_t num_components;            /* >= 1 */
    int32_t has_components;            /* 0/1 */
} ghx_field_desc;

/* One iteration space in the field's local coordinates: pattern::iteration_space_pair::local()
 * (include/ghex/structured/pattern.hpp:44-120). Only the spatial dims are given; the component
 * axis is added as [0, num_components-1] (regular/field_descriptor.hpp:131-150). */
typedef struct ghx_box
{
    int32_t first[GHX_MAX_DIM];
    int32_t last[GHX_MAX_DIM];
} ghx_box;

/* One (field, list of iteration spaces) placed into one buffer at a byte offset: the
 * communication object's field_info (include/ghex/communication_object.hpp:176-188, 1059-1065). */
typedef struct ghx_pack_entry
{
    ghx_field_desc field;
    int32_t field_slot;                /* index into field_ptrs[] at execution */
    int32_t buffer_slot;               /* index into buffer_ptrs[] at execution */
    uint64_t buffer_offset;            /* byte offset of this field's data in that buffer */
    const ghx_box* boxes;              /* iteration spaces, in pattern order */
    int32_t n_boxes;
} ghx_pack_entry;

typedef struct ghx_plan ghx_plan;

/* Build a fused pack (direction 0) or unpack (direction 1) plan over many fields, iteration
 * spaces and buffers: ONE kernel launch per execution. Replaces the per-iteration-space launch
 * loop of regular::field_descriptor::pack/unpack (include/ghex/structured/regular/field_descriptor.hpp:72-96)
 * -> serialization<gpu,L>::pack/unpack (include/ghex/structured/pack_kernels.hpp:161-248), the
 * batched pack_kernel_u of packer<gpu>::pack_u (include/ghex/packer.hpp:98-121, 192-297), and
 * packer<gpu>::pack/unpack over all buffers of communication_object::pack
 * (include/ghex/communication_object.hpp:568-597; packer.hpp:124-190).
 * The packed byte layout is bit-identical to serialization<cpu>::pack_batch. Descriptor tables
 * are uploaded to device memory here (synchronously); execution never allocates. */
int ghx_plan_create(const ghx_pack_entry* entries, int32_t n_entries, int32_t direction,
                    ghx_plan** out);
/* Enqueue the plan on `stream`: pack = buffers <- fields, unpack = fields <- buffers.
 * field_ptrs/buffer_ptrs are device pointers indexed by slot (n_field_ptrs/n_buffer_ptrs must
 * cover every slot the plan uses). */
int ghx_plan_execute(const ghx_plan* plan, void* const* field_ptrs, int32_t n_field_ptrs,
                     void* const* buffer_ptrs, int32_t n_buffer_ptrs, ghx_stream stream);
int ghx_plan_destroy(ghx_plan* plan);
/* Plan facts: total buffer bytes moved per execution, number of segments (field x iteration
 * space), number of workgroup tiles, and the largest byte offset+size touched per buffer slot. */
int ghx_plan_info(const ghx_plan* plan, uint64_t* bytes, int32_t* n_segments, int32_t* n_tiles);

/* What the planner decided for one segment (introspection only; no reference counterpart): the
 * host copy of segment k of a plan, k in [0, n_segments) of ghx_plan_info — the segments of all
 * launch groups in plan order (entries, their boxes, the pieces of a box split below 2^31 bytes).
 * A segment is `bytes / row_bytes` rows of `row_bytes` contiguous field bytes; row r sits at
 * field_off + sum_k c_k * stride[k] with r = c_0 + ext[0] * (c_1 + ext[1] * (c_2 + ext[2] * c_3))
 * and at buf_off + r * row_bytes in its buffer. wlog2: log2 of the widest vector the planner
 * allows (the launch narrows it by the pointers' alignment); amode: the field-offset arithmetic
 * the kernels take for it, 0 = general (int64), 1 / 2 = the short form ("fast_addr") with one /
 * two divisions; pipe: unpack tiles software-pipelined. Slots are the caller's. Works on plans
 * created without a device. k out of range: GHX_ERR_INVALID. */
typedef struct ghx_segment_info
{
    int64_t field_off;
    uint64_t buf_off;
    int64_t stride[4];
    uint32_t ext[4];
    uint32_t row_bytes;
    uint32_t bytes;
    uint32_t tile_bytes;
    int32_t field_slot;
    int32_t buffer_slot;
    int32_t n_outer;
    int32_t wlog2;
    int32_t amode;
    int32_t pipe;
} ghx_segment_info;
int ghx_plan_segment(const ghx_plan* plan, int32_t k, ghx_segment_info* out);

/* The reference's field.pack(T* buffer, const IndexContainer& c, void* arg)
 * (include/ghex/structured/regular/field_descriptor.hpp:72-83) for ONE field: iteration spaces
 * back to back from `buffer`. Convenience form of plan_create+execute (the descriptor upload is
 * stream-ordered from a pinned staging copy; prefer a cached plan in a loop). */
int ghx_structured_pack(const ghx_field_desc* field, const void* field_data, void* buffer,
                        const ghx_box* boxes, int32_t n_boxes, ghx_stream stream);
/* field.unpack(const T* buffer, const IndexContainer& c, void* arg)
 * (include/ghex/structured/regular/field_descriptor.hpp:85-96). */
int ghx_structured_unpack(const ghx_field_desc* field, void* field_data, const void* buffer,
                          const ghx_box* boxes, int32_t n_boxes, ghx_stream stream);

/* ------------------------------------------------------------------------------------------
 * Unstructured fields (index-list gather / scatter)
 * ------------------------------------------------------------------------------------------ */

/* unstructured::data_descriptor<gpu> (include/ghex/unstructured/user_concepts.hpp:526-577):
 * value(lid, level) at values + (lid*index_stride + level*level_stride)*elem_size. */
typedef struct ghx_udata_desc
{
    int32_t elem_size;
    int32_t levels;
    int32_t levels_first;              /* buffer order: levels_first ? [i][level] : [level][i] */
    int64_t index_stride;              /* in elements */
    int64_t level_stride;              /* in elements */
} ghx_udata_desc;

typedef struct ghx_upack_entry
{
    ghx_udata_desc data;
    int32_t field_slot;
    int32_t buffer_slot;
    uint64_t buffer_offset;
    const int64_t* lids;               /* HOST array of local indices (pattern order); copied to
                                          device memory as int32 (int64 if any lid >= 2^31) */
    int64_t n_lids;
} ghx_upack_entry;

typedef struct ghx_uplan ghx_uplan;

/* The reference's data_descriptor<gpu>::pack/unpack(T* buffer, const IndexContainer& c, void*
 * stream) for ONE index list (include/ghex/unstructured/user_concepts.hpp:583-666): gather
 * values[lids[i]] (all levels, the descriptor's layout) into `buffer` / scatter back. `lids` is
 * a HOST-readable array of int32 (lid_bytes 4) or int64 (8) local indices, e.g. the pattern's
 * iteration_space::local_indices(). Plans are cached by (descriptor, list address, length); a
 * hit compares the whole list with the copy the plan was built from, so a list changed in place
 * gets a new plan. Replaced plans are freed once their last execution has completed (never with
 * a device-wide synchronisation); plans executed inside a stream capture are kept alive. */
int ghx_unstructured_pack(const ghx_udata_desc* data, const void* values, void* buffer,
                          const void* lids, int32_t lid_bytes, int64_t n_lids, ghx_stream stream);
int ghx_unstructured_unpack(const ghx_udata_desc* data, void* values, const void* buffer,
                            const void* lids, int32_t lid_bytes, int64_t n_lids, ghx_stream stream);

/* Fused unstructured pack (0) / unpack (1) plan: replaces data_descriptor<gpu>::pack/unpack
 * and the four pack/unpack_kernel_levels_{first,last} launches per neighbour
 * (include/ghex/unstructured/user_concepts.hpp:455-523, 583-666). Index lists live in
 * device memory (not managed memory as in unstructured/pattern.hpp:53-57). */
int ghx_uplan_create(const ghx_upack_entry* entries, int32_t n_entries, int32_t direction,
                     ghx_uplan** out);
int ghx_uplan_execute(const ghx_uplan* plan, void* const* field_ptrs, int32_t n_field_ptrs,
                      void* const* buffer_ptrs, int32_t n_buffer_ptrs, ghx_stream stream);
int ghx_uplan_destroy(ghx_uplan* plan);
int ghx_uplan_info(const ghx_uplan* plan, uint64_t* bytes, int32_t* n_segments, int32_t* n_tiles);

/* What the planner decided for one index-list segment (introspection only, the twin of
 * ghx_plan_segment): the host copy of segment k of a plan, k in [0, n_segments) of
 * ghx_uplan_info — the segments of all launch groups in plan order (entries, the pieces of a
 * list split below 2^30 bytes). A segment moves `bytes` buffer bytes from buf_off on, as rows of
 * `row_bytes` contiguous field bytes over `n` local indices. Buffer row r sits in the field at
 * field_off + lid[i] * index_stride_b + l * level_stride_b, where by `mode`
 *   0: i = r, l = 0 (one row per index: all its levels, or the one level of a split list);
 *   1: i = r / levels, l = r % levels (levels first, strided levels; levels = bytes/row_bytes/n);
 *   2: l = r / n, i = r % n (levels last).
 * tile_bytes: the segment's workgroup tile, a whole number of rows. wlog2: log2 of the widest
 * vector the planner allows (the launch narrows it by the pointers' alignment). lid64: the
 * device index table holds int64 (some lid >= 2^31), else int32. runs: the segment qualifies for
 * the run path (4/8-B rows adjacent in the field; 2: run-heavy), which a launch takes only when
 * every segment of its group does and the pointers allow it. fpol: field-side cache policy (bit 0
 * non-temporal loads, bit 1 sc1 stores). Slots are the caller's. Works on plans created without
 * a device. k out of range: GHX_ERR_INVALID. */
typedef struct ghx_usegment_info
{
    int64_t field_off;
    uint64_t buf_off;
    int64_t index_stride_b;
    int64_t level_stride_b;
    uint32_t bytes;
    uint32_t row_bytes;
    uint32_t tile_bytes;
    uint32_t n;
    int32_t field_slot;
    int32_t buffer_slot;
    int32_t mode;
    int32_t wlog2;
    int32_t lid64;
    int32_t runs;
    int32_t fpol;
} ghx_usegment_info;
int ghx_uplan_segment(const ghx_uplan* plan, int32_t k, ghx_usegment_info* out);

/* ------------------------------------------------------------------------------------------
 * Patterns (setup time, host only): the producers of the pack inputs.
 * ------------------------------------------------------------------------------------------ */

/* One rank's domains for pattern construction, given for ALL ranks (the reference obtains them
 * with MPI all_gather, include/ghex/structured/pattern.hpp:268-273). */
typedef struct ghx_regular_domain
{
    int32_t id;
    int32_t rank;
    int32_t first[3];
    int32_t last[3];
} ghx_regular_domain;

typedef struct ghx_pattern ghx_pattern;

/* halo_generator::operator() (include/ghex/structured/regular/halo_generator.hpp:93-148):
 * receive boxes of one domain, in the reference's order. Writes up to max_boxes boxes
 * (local first/last into `local`, global first/last into `global`), returns the count in
 * *n_boxes (call with max_boxes = 0 to query). halos = (dim0-, dim0+, dim1-, dim1+, ...). */
int ghx_regular_halo_boxes(int32_t dim, const int32_t* global_first, const int32_t* global_last,
                           const int32_t* halos, const int32_t* periodic,
                           const int32_t* domain_first, const int32_t* domain_last,
                           ghx_box* local, ghx_box* global, int32_t max_boxes, int32_t* n_boxes);

/* make_pattern<structured::grid> (include/ghex/structured/pattern.hpp:214-571), computed for
 * rank `my_rank` from all ranks' domains (ordered by rank, then each rank's d_range order). */
int ghx_regular_pattern_create(int32_t dim, const ghx_regular_domain* domains,
                               int32_t n_domains, const int32_t* global_first,
                               const int32_t* global_last, const int32_t* halos,
                               const int32_t* periodic, int32_t my_rank, ghx_pattern** out);

/* make_staged_pattern (include/ghex/structured/regular/make_pattern.hpp:47-250): `dim` pattern
 * handles written to out[0..dim-1], stage i exchanging the halos of dimension i over the domain
 * box extended by the halos of stages 0..i-1 (exchanging the stages in order fills edges and
 * corners). domains as for ghx_regular_pattern_create (all ranks); neighbors[(k*dim + i)*2 + s]
 * = the id of domain k's left (s = 0) / right (s = 1) neighbour in dimension i — the reference's
 * domain look-up `d_lu(id, offset)` evaluated for offset -1/+1 along i; only consulted where
 * that side has a halo (non-zero width, and periodic or inside the global box). */
int ghx_staged_pattern_create(int32_t dim, const ghx_regular_domain* domains, int32_t n_domains,
                              const int32_t* neighbors, const int32_t* global_first,
                              const int32_t* global_last, const int32_t* halos,
                              const int32_t* periodic, int32_t my_rank, ghx_pattern** out);

/* unstructured::domain_descriptor(id, gids, outer lids) (include/ghex/unstructured/
 * user_concepts.hpp:37-176): gids in storage order, the local ids of the outer (halo) cells.
 * Builds the gid -> lid maps (flat hash tables) once; immutable afterwards (shareable between
 * threads). Fails (GHX_ERR_PATTERN) on a repeated outer lid or a repeated inner gid, like the
 * reference's constructor. */
typedef struct ghx_udomain ghx_udomain;
int ghx_udomain_create(int32_t id, const int64_t* gids, int64_t n_gids, const int64_t* outer_lids,
                       int64_t n_outer, ghx_udomain** out);
int ghx_udomain_destroy(ghx_udomain* d);
int ghx_udomain_info(const ghx_udomain* d, int32_t* id, int64_t* size, int64_t* inner_size,
                     int64_t* n_outer);
/* halo_generator::operator() (user_concepts.hpp:234-256) as gids: the domain's reduced halo, i.e.
 * the gids of make_outer_lids(gen_gids) (n_gen < 0: all outer gids in storage order). Writes
 * *n_halo <= max(n_gen, n_outer) gids; cap must hold them. */
int ghx_udomain_halo(const ghx_udomain* d, const int64_t* gen_gids, int64_t n_gen,
                     int64_t* halo_gids, int64_t cap, int64_t* n_halo);

/* make_pattern<unstructured::grid> (include/ghex/unstructured/pattern.hpp:187-370) for ONE rank,
 * in the reference's three steps; the caller moves the bytes between ranks (only halo gids ever
 * travel, never a rank's full gid list):
 *   1. ghx_upattern_create with this rank's domains and the global max domain count per rank and
 *      max domain id (the tag layout, :218-233);
 *   2. ghx_upattern_add_halos once per rank r (this one included; any order) with r's domain ids
 *      and reduced halos (ghx_udomain_halo, concatenated): creates this rank's send halos for
 *      every halo gid that is an inner cell of one of its domains (:284-330) and a record per
 *      (my domain, r's domain) pair whose gid list must reach rank dst_rank (ghx_upattern_record:
 *      the pointer stays valid until ghx_upattern_destroy);
 *   3. ghx_upattern_add_recv for every record addressed to this rank (src = the record's sender):
 *      make_outer_lids -> receive halos (:337-365); then ghx_upattern_finish.
 * Maps are keyed and ordered (rank, tag) as the reference's (pattern.hpp:105-110). */
typedef struct ghx_upattern ghx_upattern;
int ghx_upattern_create(const ghx_udomain* const* domains, int32_t n_domains, int32_t my_rank,
                        int32_t max_num_domains, int32_t max_domain_id, ghx_upattern** out);
int ghx_upattern_add_halos(ghx_upattern* b, int32_t rank, int32_t n_domains,
                           const int32_t* domain_ids, const int64_t* halo_sizes,
                           const int64_t* halo_gids, int64_t* n_records);
int ghx_upattern_record(const ghx_upattern* b, int64_t k, int32_t* src_id, int32_t* dst_id,
                        int32_t* dst_rank, int32_t* tag, int64_t* n_gids, const int64_t** gids);
int ghx_upattern_add_recv(ghx_upattern* b, int32_t src_rank, int32_t src_id, int32_t dst_id,
                          int32_t tag, const int64_t* gids, int64_t n_gids);
int ghx_upattern_finish(ghx_upattern* b, ghx_pattern** out);
int ghx_upattern_destroy(ghx_upattern* b);

int ghx_pattern_destroy(ghx_pattern* p);
/* A copy of a pattern whose send and receive halo maps keep only the keys whose remote rank is
 * in `ranks` (keep = 1) or is not (keep = 0); tags and max_tag unchanged. The bulk exchange
 * splits a pattern this way into its node-local part (puts) and its remote part (a buffered
 * exchange), as the reference's bulk object splits it into local and remote pattern maps
 * (include/ghex/bulk_communication_object.hpp:330-383). */
int ghx_pattern_filter(const ghx_pattern* p, const int32_t* ranks, int32_t n_ranks, int32_t keep,
                       ghx_pattern** out);
/* Number of local domains (patterns) of this rank, and the global max tag
 * (pattern_container::max_tag, include/ghex/pattern_container.hpp:78-83). */
int ghx_pattern_num_domains(const ghx_pattern* p, int32_t* n);
int ghx_pattern_max_tag(const ghx_pattern* p, int32_t* max_tag);
int ghx_pattern_domain_id(const ghx_pattern* p, int32_t local_index, int32_t* id);
/* Halo maps of local domain `local_index`: direction 0 = send_halos(), 1 = recv_halos(),
 * in std::map key order. Key k: remote domain id, remote rank, tag, #iteration spaces and
 * #elements (spatial). */
int ghx_pattern_num_keys(const ghx_pattern* p, int32_t local_index, int32_t direction,
                         int32_t* n_keys);
int ghx_pattern_key(const ghx_pattern* p, int32_t local_index, int32_t direction, int32_t key,
                    int32_t* remote_id, int32_t* remote_rank, int32_t* tag, int32_t* n_spaces,
                    int64_t* n_elements);
/* Structured: the iteration spaces of a key (local and global boxes). */
int ghx_pattern_key_boxes(const ghx_pattern* p, int32_t local_index, int32_t direction,
                          int32_t key, ghx_box* local, ghx_box* global, int32_t max_boxes);
/* Unstructured: the local index list of a key (its single iteration space). */
int ghx_pattern_key_lids(const ghx_pattern* p, int32_t local_index, int32_t direction,
                         int32_t key, int64_t* lids, int64_t max_lids);

/* ------------------------------------------------------------------------------------------
 * Cubed-sphere grids (include/ghex/structured/cubed_sphere/): six tiles of edge_size x edge_size
 * cells over `levels` levels, oriented as drawn in cubed_sphere/transform.hpp:21-38. A halo that
 * crosses a cube edge arrives in the neighbour tile's coordinates and is rotated (and, for
 * vector fields, sign-flipped) into the receiver's by the unpack
 * (cubed_sphere/field_descriptor.hpp:55-109, 142-167).
 * ------------------------------------------------------------------------------------------ */

/* cubed_sphere::domain_descriptor(cube, tile, x_first, x_last, y_first, y_last)
 * (cubed_sphere/domain_descriptor.hpp:92-104) of one rank; all levels. The library computes
 * the domain's int32 id as (tile * edge_size + y_first) * edge_size + x_first, whose integer
 * order is the order of the reference's (tile, (x_first, y_first)) ids (:33-61). */
typedef struct ghx_cs_domain
{
    int32_t rank;
    int32_t tile;
    int32_t x_first, x_last;
    int32_t y_first, y_last;
} ghx_cs_domain;

/* cubed_sphere::halo_generator::operator() (cubed_sphere/halo_generator.hpp:75-198): the receive
 * boxes of one domain in the reference's order, local and global coordinates (x, y, z) and the
 * tile of each global box (the domain's own or an edge neighbour's, whose coordinates the
 * global box is then given in). halos = the four widths as the code applies them: -x, +x, -y,
 * +y. Query the count with max_boxes = 0. `rank` of the domain is ignored. */
int ghx_cs_halo_boxes(int32_t edge_size, int32_t levels, const ghx_cs_domain* domain,
                      const int32_t* halos, ghx_box* local, ghx_box* global, int32_t* tiles,
                      int32_t max_boxes, int32_t* n_boxes);

/* make_pattern<structured::grid> (include/ghex/structured/pattern.hpp:214-571) with the
 * cubed-sphere halo generator and its seven-argument intersect (halo_generator.hpp:227-283),
 * for rank `my_rank` from ALL ranks' domains (ordered by rank, then each rank's d_range order).
 * The result is an ordinary 3-D structured pattern (every ghx_pattern_* query works on it);
 * ghx_pattern_key_tiles adds the tile of each iteration space's global box. Send boxes are in
 * the sender's coordinates, so packing is the ordinary pack. */
int ghx_cs_pattern_create(int32_t edge_size, int32_t levels, const ghx_cs_domain* domains,
                          int32_t n_domains, const int32_t* halos, int32_t my_rank,
                          ghx_pattern** out);
/* The tile of the global box of each iteration space of a key (same order as
 * ghx_pattern_key_boxes); GHX_ERR_INVALID on a pattern that is not a cubed-sphere one. */
int ghx_pattern_key_tiles(const ghx_pattern* p, int32_t local_index, int32_t direction,
                          int32_t key, int32_t* tiles, int32_t max_boxes);

/* ------------------------------------------------------------------------------------------
 * Exchange planning: communication_object::allocate semantics (buffer per domain pair, fields
 * in exchange() order, alignof padding, tag = pattern tag + container tag offset)
 * (include/ghex/communication_object.hpp:483-566, 1003-1067).
 * ------------------------------------------------------------------------------------------ */

typedef struct ghx_exchange_item
{
    const ghx_pattern* pattern;        /* the field's pattern container (this rank) */
    int32_t local_index;               /* which local domain of that pattern */
    int32_t kind;                      /* 0 = structured (field), 1 = unstructured (udata) */
    ghx_field_desc field;              /* kind 0 */
    ghx_udata_desc udata;              /* kind 1 */
    int32_t align;                     /* alignof(value_type) */
    int32_t tag_offset;                /* prepare_exchange_buffers tag map (:540-549) */
} ghx_exchange_item;

typedef struct ghx_exchange ghx_exchange;

/* Plans one exchange() of n_items fields (field_slot = item index). Produces the send and recv
 * buffer lists (std::map order of domain_id_pair) and fused pack / unpack plans over them
 * (buffer_slot = buffer index). */
int ghx_exchange_create(const ghx_exchange_item* items, int32_t n_items, ghx_exchange** out);
int ghx_exchange_destroy(ghx_exchange* ex);
/* direction 0 = send buffers, 1 = recv buffers. */
int ghx_exchange_num_buffers(const ghx_exchange* ex, int32_t direction, int32_t* n);
int ghx_exchange_buffer(const ghx_exchange* ex, int32_t direction, int32_t index,
                        int32_t* first_id, int32_t* second_id, int32_t* rank, int32_t* tag,
                        uint64_t* size);
/* Enqueue the fused pack of all send buffers / fused unpack of all recv buffers. */
int ghx_exchange_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                      void* const* send_buffers, int32_t n_send, ghx_stream stream);
int ghx_exchange_unpack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                        void* const* recv_buffers, int32_t n_recv, ghx_stream stream);

/* Per-buffer plans: ghx_exchange_split builds one pack and one unpack plan per buffer (setup
 * time, synchronous upload); ghx_exchange_pack_buffer / ghx_exchange_unpack_buffer then enqueue
 * the pack of send buffer `index` / the unpack of recv buffer `index` alone, with the same
 * pointer arrays as ghx_exchange_pack/unpack. This is the reference's per-buffer packer call on
 * the buffer's own stream (include/ghex/communication_object.hpp:568-597, packer.hpp:124-190),
 * used to send each message as soon as its own pack is done (:611-637). */
int ghx_exchange_split(ghx_exchange* ex);
int ghx_exchange_pack_buffer(const ghx_exchange* ex, int32_t index, void* const* field_ptrs,
                             int32_t n_fields, void* const* send_buffers, int32_t n_send,
                             ghx_stream stream);
int ghx_exchange_unpack_buffer(const ghx_exchange* ex, int32_t index, void* const* field_ptrs,
                               int32_t n_fields, void* const* recv_buffers, int32_t n_recv,
                               ghx_stream stream);

/* ------------------------------------------------------------------------------------------
 * RCCL transport (one rank per GPU, xGMI inside a node): replaces oomph's NCCL backend
 * (start_group/send/recv/end_group, include/ghex/communication_object.hpp:278-281, 641-714).
 * RCCL is loaded at run time from `path` (NULL: "librccl.so.1") — pass the library the process
 * already uses (torch's), so one RCCL instance serves both.
 * ------------------------------------------------------------------------------------------ */
int ghx_rccl_open(const char* path);
int ghx_rccl_unique_id(unsigned char id[128]);
/* ncclCommInitRank (blocking until all `nranks` ranks have called it). */
int ghx_rccl_comm_init(const unsigned char id[128], int32_t nranks, int32_t rank, void** comm);
int ghx_rccl_comm_destroy(void* comm);
/* GHX_OK, or the communicator's asynchronous error as GHX_ERR_HIP. */
int ghx_rccl_comm_check(void* comm);

/* Per-peer pipelined exchange (the reference's per-buffer streams + send-as-packed,
 * include/ghex/device/cuda/stream.hpp:25-73, communication_object.hpp:568-637, 703-767): for
 * each peer, in the given order, on its own greatest-priority stream: pack of its send buffers,
 * one RCCL group {recv..., send...} on comms[k] (the peer is rank comm_ranks[k] there), unpack of
 * its recv buffers. Messages of one pair are issued in (tag, domain pair) order on both sides.
 * Peer k rides stream k mod max_streams (the device has few hardware queues, 4 by default:
 * streams beyond them share queues in an order no one chooses; dealt this way every stream
 * still runs its peers in the global order). Buffers of ranks not listed must be self messages
 * (my_rank): packed and unpacked on the
 * caller's stream. ghx_pipeline_run enqueues all of it; the caller's stream then waits for every
 * peer stream (no host synchronisation). Every rank must list its peers in one global order
 * consistent across ranks (e.g. round-robin tournament rounds) so that no wait cycle can form
 * when streams share hardware queues. Not re-entrant: one run at a time per pipeline. */
typedef struct ghx_pipeline ghx_pipeline;
int ghx_pipeline_create(ghx_exchange* ex, int32_t my_rank, int32_t n_peers,
                        const int32_t* peer_ranks, void* const* comms, const int32_t* comm_ranks,
                        int32_t max_streams, ghx_pipeline** out);
int ghx_pipeline_run(const ghx_pipeline* pl, void* const* field_ptrs, int32_t n_fields,
                     void* const* send_buffers, int32_t n_send, void* const* recv_buffers,
                     int32_t n_recv, ghx_stream stream);
int ghx_pipeline_destroy(ghx_pipeline* pl);

/* Self messages (a periodic wrap onto the same rank, or two domains of one rank) never leave
 * the device in the reference's stream-aware flow either (communication_object.hpp:703-767:
 * pack -> send to self -> unpack). When EVERY message of an exchange is a self message
 * (*fusable = 1), ghx_exchange_self performs pack and unpack in ONE launch: each workgroup packs
 * a tile of the send buffer and then writes the same bytes into the halos (from the registers it
 * stored them from, or after a workgroup barrier). The buffers are the send buffers (they double
 * as recv buffers); every packed byte and every halo byte is written, and the send buffers hold
 * the packed message afterwards. */
int ghx_exchange_self_fusable(const ghx_exchange* ex, int32_t* fusable);
int ghx_exchange_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                      void* const* buffers, int32_t n_buffers, ghx_stream stream);

/* Exchanges with self messages AND peer messages (*mixed = 1; e.g. a (2,1,1) periodic
 * decomposition: x to the neighbour, y and z onto the rank itself): ghx_exchange_pack_self packs
 * every send buffer AND completes the self messages (their halos written in the same launch);
 * the transport then carries the peer messages only, and ghx_exchange_unpack_peers unpacks the
 * peer recv buffers only (same pointer arrays as ghx_exchange_pack/unpack). Together they do
 * exactly what ghx_exchange_pack + ghx_exchange_unpack do. */
int ghx_exchange_mixed(const ghx_exchange* ex, int32_t* mixed);
int ghx_exchange_pack_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                           void* const* send_buffers, int32_t n_send, ghx_stream stream);
int ghx_exchange_unpack_peers(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                              void* const* recv_buffers, int32_t n_recv, ghx_stream stream);

/* Double-buffered buffers (the direct exchange's one-launch epochs, ghx_epochs_enqueue phase 2):
 * every later pack (direction 0: ghx_exchange_pack, _pack_self, _pack_buffer) or unpack (1:
 * ghx_exchange_unpack, _unpack_peers, _unpack_buffer) launch of `ex` uses, for buffer i with
 * offsets[i] != 0, the copy at
 * buffer_ptr + offsets[i] when (*parity_word + parity_add) is odd, read on the device at launch
 * (a captured graph alternates on replay). offsets: one per buffer of that direction, multiples
 * of 256 B (0 = one copy). parity_word = NULL restores single buffers. The reference has no
 * equivalent (its RMA path puts field to field, include/ghex/structured/rma_put.hpp:204-245). */
int ghx_exchange_set_parity(ghx_exchange* ex, int32_t direction, const uint64_t* parity_word,
                            uint32_t parity_add, const int64_t* offsets, int32_t n_buffers);

/* Cubed-sphere exchanges. cs_items[i] goes with items[i] (a structured item whose pattern came
 * from ghx_cs_pattern_create): the field's domain (tile, first x / y cell, the cube's edge
 * size), is_vector (cubed_sphere::field_descriptor's is_vector_field) and the value kind that
 * says how a vector component is negated: 0 = opaque bits (scalar fields only), 1 = IEEE float
 * of elem_size 4 / 8 (sign-bit flip), 2 = signed integer of elem_size 4 / 8 (two's-complement
 * negate). A vector field of any other value type is refused (GHX_ERR_INVALID).
 * The result is an ordinary ghx_exchange: buffers, sizes, tags and ghx_exchange_pack are those
 * of ghx_exchange_create; ghx_exchange_unpack enqueues the ordinary unpack launch and then, on
 * the same stream, the transformed one (k_unpack_x) for the spaces received from another tile
 * whose rotation moves or reverses the field's stride-1 axis or negates a component. Rotated
 * spaces that keep contiguous rows (z or the component stride-1) ride the ordinary launch.
 * With one transformed (rotated) space ghx_exchange_self_fusable and ghx_exchange_mixed report
 * 0, and ghx_exchange_split and ghx_exchange_set_parity(direction 1) fail with GHX_ERR_INVALID:
 * the per-buffer, pipelined and double-buffered unpacks do not rotate. ghx_put_create sees
 * fields and boxes only and refuses a rotated pair of boxes: puts from a cubed-sphere pattern
 * are built with ghx_cs_put_create (below, with the other put entry points), which takes the
 * receiver's cubed-sphere item, global boxes and tiles as well. */
typedef struct ghx_cs_item
{
    int32_t tile;
    int32_t first_x, first_y;
    int32_t edge_size;
    int32_t is_vector;
    int32_t value_kind;
} ghx_cs_item;
int ghx_cs_exchange_create(const ghx_exchange_item* items, const ghx_cs_item* cs_items,
                           int32_t n_items, ghx_exchange** out);
/* The transformed part of an exchange's unpack (ghx_plan_info / ghx_plan_segment describe the
 * ordinary part only): number of transformed-segment records (one per rotated iteration space
 * and field), their buffer bytes and workgroup tiles, and the number of rotated spaces in all
 * (those planned as ordinary segments included). Works on exchanges created without a device. */
int ghx_cs_plan_info(const ghx_exchange* ex, int32_t* n_records, uint64_t* bytes,
                     int32_t* n_tiles, int32_t* n_rotated);
/* The fused self exchange of a cubed-sphere exchange. When every message stays on this rank
 * (every recv buffer is the send buffer of the same domain pair: a whole cube on one rank), all
 * items fit one launch (fields and send buffers together at most 448 pointers: the launch has
 * a pointer table of its own, not the GHX_MAX_SLOTS of the other launches), the two fields of every
 * message agree in element size, components and layout order, and no send box reaches into a
 * halo the exchange writes, ghx_cs_exchange_create also plans ONE launch (k_self_cs) that does
 * what ghx_exchange_pack + ghx_exchange_unpack do: spaces whose pack and unpack segments cover the
 * same bytes with the same rows run as ghx_exchange_self runs them (*n_pair_tiles workgroup
 * tiles); the others (*n_x_records spaces: the transformed ones, and ordinary ones whose rows
 * differ between the two sides) run element by element, sending field -> buffer and -> receiving
 * field, rotated and negated in registers (*n_x_tiles tiles). ghx_cs_self_info works without a
 * device; with *fusable = 0, ghx_last_error() holds the reason. ghx_cs_exchange_self has
 * ghx_exchange_self's argument contract (the buffers are the send buffers, which hold the packed
 * message afterwards) and fails with GHX_ERR_INVALID on an exchange that is not fusable or whose
 * send side has parity set (ghx_exchange_set_parity, direction 0). ghx_exchange_self_fusable,
 * ghx_exchange_mixed and the refusals above are unchanged by it. */
int ghx_cs_self_info(const ghx_exchange* ex, int32_t* fusable, int32_t* n_pair_tiles,
                     int32_t* n_x_records, int32_t* n_x_tiles);
int ghx_cs_exchange_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                         void* const* buffers, int32_t n_buffers, ghx_stream stream);
/* cubed_sphere::field_descriptor::unpack(const T* buffer, const IndexContainer& c, void* arg)
 * (cubed_sphere/field_descriptor.hpp:142-167) for ONE field: iteration spaces back to back from
 * `buffer`, each with its local box, global box and the global box's tile. Convenience form
 * (cached plan), next to ghx_structured_unpack. */
int ghx_cs_unpack(const ghx_field_desc* field, const ghx_cs_item* cs, void* field_data,
                  const void* buffer, const ghx_box* local, const ghx_box* global,
                  const int32_t* tiles, int32_t n_boxes, ghx_stream stream);
/* The transpose of ghx_cs_unpack for ONE field, with the same arguments and the same cached plan:
 * the field is READ and the buffer is WRITTEN. Every cell of every local box goes to the buffer
 * position ghx_cs_unpack reads it from, negated where ghx_cs_unpack negates (the sign matrix is
 * diagonal: its transpose is itself), so ghx_cs_unpack(ghx_cs_pack_rotated(R)) restores the boxes
 * of R bit for bit. Ordinary spaces run a pack launch, transformed ones k_pack_x over the
 * records k_unpack_x reads. Every element size ghx_cs_unpack takes. The reference has no
 * counterpart (its cubed-sphere descriptor packs unrotated, field_descriptor.hpp:110-140). */
int ghx_cs_pack_rotated(const ghx_field_desc* field, const ghx_cs_item* cs, const void* field_data,
                        void* buffer, const ghx_box* local, const ghx_box* global,
                        const int32_t* tiles, int32_t n_boxes, ghx_stream stream);

/* ------------------------------------------------------------------------------------------
 * Zero-copy put between node-local GPUs. Replaces the reference's RMA path:
 * bulk_communication_object (include/ghex/bulk_communication_object.hpp:206-704), the
 * gpu_to_gpu put (include/ghex/structured/rma_put.hpp:204-245: one launch per range, one
 * element per thread) and the CUDA IPC handles (include/ghex/rma/cuda/handle.hpp:20-96).
 * ------------------------------------------------------------------------------------------ */

/* Export the device allocation holding `ptr` for another process: a 64-byte IPC handle of the
 * allocation's base and the byte offset of `ptr` inside it (torch's caching allocator hands out
 * interior pointers). */
int ghx_ipc_export(const void* ptr, unsigned char handle[64], uint64_t* offset);
/* Map another process's allocation: *base is what ghx_ipc_close releases, *ptr = base+offset. */
int ghx_ipc_import(const unsigned char handle[64], uint64_t offset, void** base, void** ptr);
int ghx_ipc_close(void* base);

/* A put plan: src[k] and dst[k] describe the two ends of the same virtual message bytes — the
 * iteration spaces of a sender's send halo (its local coordinates, its field) and of the
 * receiver's recv halo for the same key (the receiver's coordinates and field), each entry's
 * buffer_slot/buffer_offset placing it in a virtual message exactly as ghx_plan_create would.
 * Field slots: src entries index src_fields, dst entries index dst_fields (< 64 each: one
 * launch; the bulk objects group their messages into several put plans).
 * Execution copies every element straight from the source field into the target field (peer
 * memory through ghx_ipc_import, or the same device): no buffer, one launch. Fails with
 * GHX_ERR_INVALID when the two sides do not describe the same bytes. */
typedef struct ghx_put ghx_put;
int ghx_put_create(const ghx_pack_entry* src, int32_t n_src, const ghx_pack_entry* dst,
                   int32_t n_dst, ghx_put** out);
int ghx_put_execute(const ghx_put* put, void* const* src_fields, int32_t n_src,
                    void* const* dst_fields, int32_t n_dst, ghx_stream stream);
int ghx_put_info(const ghx_put* put, uint64_t* bytes, int32_t* n_tiles);
int ghx_put_destroy(ghx_put* put);

/* A put plan over cubed-sphere fields (no reference counterpart: the reference's RMA put does not
 * rotate). src and dst are ghx_put_create's two entry arrays — the source side is the ordinary
 * pack side of a cubed-sphere exchange, a box of the sender's field in its own coordinates, and
 * needs no cubed-sphere item. Per target entry k: dst_cs[k], the receiving field's item as for
 * ghx_cs_exchange_create; dst_global[k][b] and dst_tiles[k][b], the global box of the entry's
 * b-th space and that box's tile (ghx_pattern_key_boxes / ghx_pattern_key_tiles of the
 * receiver's recv halo). Each target space is paired with the source space at the same virtual
 * message bytes (buffer_slot, running offset). Spaces the receiver would unpack as ordinary
 * segments whose rows the sender's segments match one to one run as ghx_put_create's do
 * (*n_pair_tiles workgroup tiles); every other space (*n_x_records of them: the transformed
 * ones, and ordinary ones whose rows differ between the two sides) runs element by element —
 * sending field -> receiving field, rotated and negated in registers (*n_x_tiles tiles; the
 * "x_tile_elems" knob sizes them) — in the same single launch (k_put_cs). Element-wide accesses
 * where both pointers and all strides are element-aligned at run time, byte-wide otherwise.
 * The result is an ordinary ghx_put for ghx_put_execute / ghx_put_info (bytes = the message
 * bytes, tiles of both kinds) / ghx_put_destroy, with the same limit of fewer than 64 source
 * and 64 target field slots, and can be created without a device.
 * GHX_ERR_INVALID, with the reason in ghx_last_error(), when: the two fields of a message differ
 * in element size, components or layout order; a space that cannot be paired holds elements that
 * are not 1, 2, 4, 8 or 16 bytes; a source box and its target box differ in shape under the tile
 * transform; a vector field's value kind is one ghx_cs_exchange_create refuses; a source box
 * starts below local cell 0 on any axis (it would read the sender's halo, which the sender's own
 * sources write in the same epoch). ghx_cs_put_info on a plan of ghx_put_create reports its
 * tiles as pair tiles and zeros for the transformed part. */
int ghx_cs_put_create(const ghx_pack_entry* src, int32_t n_src, const ghx_pack_entry* dst,
                      int32_t n_dst, const ghx_cs_item* dst_cs, const ghx_box* const* dst_global,
                      const int32_t* const* dst_tiles, ghx_put** out);
int ghx_cs_put_info(const ghx_put* put, int32_t* n_pair_tiles, int32_t* n_x_records,
                    int32_t* n_x_tiles);

/* A put plan over unstructured fields (no reference counterpart: the reference's bulk object is
 * structured only). src[k] and dst[k] are the two ends of message k: a sender's send list on its
 * field and the receiver's receive list for the same key on its field (ghx_pattern_key_lids of
 * either side), n messages. Field slots: src entries index src_fields, dst entries dst_fields
 * (< 64 each: one launch, no launch groups; the bulk object groups its messages into several put
 * plans). Execution performs, for every i < n_lids and l < levels,
 *   dst.values[(t[i]*dst.index_stride + l*dst.level_stride)*elem] <-
 *   src.values[(s[i]*src.index_stride + l*src.level_stride)*elem]
 * (s, t: the source and target lists), byte for byte what a ghx_uplan pack of the source side
 * followed by a ghx_uplan unpack of the target side leaves in the target field — as ONE launch
 * (k_put_u) with no buffer: both index tables are read together, each value is loaded from the
 * source field and stored to the target field (this device's memory or a peer's through
 * ghx_ipc_import). Messages of 4- or 8-byte rows move 16 bytes per lane, as one 16-byte access on
 * a side whose lids form a run there (knob "urun"), as in the index-list pack. The result is an
 * ordinary ghx_put for ghx_put_execute (stream-ordered, never allocates, capturable) /
 * ghx_put_info (message bytes, workgroup tiles) / ghx_put_destroy; ghx_cs_put_info reports its
 * tiles as pair tiles and zeros for the rest. Created without a device like every other plan
 * (the tables are uploaded only when there is one; execution then reports GHX_ERR_HIP).
 * GHX_ERR_INVALID, with the reason in ghx_last_error(), when: the two sides of a message differ
 * in n_lids, elem_size, levels or levels_first (they would not describe the same message bytes:
 * the buffered path pairs bytes by position); a lid is negative; elem_size < 1 or levels < 1; a
 * slot is negative or >= 64; a row (levels * elem_size) is longer than 1 GiB.
 * Contract, not checked: no source cell of an exchange is a target cell of the same exchange, and
 * the target lids of one field are distinct (the patterns guarantee both: send lists hold inner
 * cells, receive lists outer cells). Source lids may repeat. */
typedef struct ghx_uput_entry
{
    ghx_udata_desc data;               /* this side's field */
    int32_t field_slot;
    const int64_t* lids;               /* HOST array (pattern order); copied to device memory as
                                          int32, or int64 if any lid of the list is >= 2^31 */
    int64_t n_lids;
} ghx_uput_entry;
int ghx_uput_create(const ghx_uput_entry* src, const ghx_uput_entry* dst, int32_t n, ghx_put** out);

/* What the planner decided for segment k of a plan of ghx_uput_create (host only, the twin of
 * ghx_uplan_segment): k in [0, n_segments), the messages in order, a message beyond 2^30 bytes as
 * several segments (index ranges; a levels-last list level by level) cut identically on both
 * sides. The segment covers positions [first_index, first_index + n) of both lists of message
 * `message`. Message row r of the segment sits, on either side, at that side's
 * field_off + lid[first_index + i] * index_stride_b + l * level_stride_b with (i, l) by the
 * common `mode` as for ghx_usegment_info. row_bytes, bytes, tile_bytes (whole rows) and wlog2
 * (the widest vector both sides allow; the launch narrows it by both pointers) are common;
 * lid64 and runs are per side (runs: the side may form 16-byte runs; 2: run-heavy).
 * GHX_ERR_INVALID for a put that did not come from ghx_uput_create, or k out of range. */
typedef struct ghx_uput_segment_info
{
    int64_t src_field_off, src_index_stride_b, src_level_stride_b;
    int64_t dst_field_off, dst_index_stride_b, dst_level_stride_b;
    int64_t first_index;
    uint32_t bytes;
    uint32_t row_bytes;
    uint32_t tile_bytes;
    uint32_t n;
    int32_t message;
    int32_t n_segments;                /* of the whole plan */
    int32_t src_slot, dst_slot;
    int32_t mode;
    int32_t wlog2;
    int32_t src_lid64, dst_lid64;
    int32_t src_runs, dst_runs;
} ghx_uput_segment_info;
int ghx_uput_segment(const ghx_put* put, int32_t k, ghx_uput_segment_info* out);

/* The fused self exchange of index lists (no reference counterpart: the reference packs, sends to
 * self and unpacks, communication_object.hpp:703-767). src[k] is message k's pack entry (the
 * sender's field, its send list, buffer_slot and buffer_offset) and dst[k] the unpack entry of
 * the SAME message bytes (the receiver's field, its receive list; buffer_slot and buffer_offset
 * equal src[k]'s). The field slots of both sides index ONE field pointer array (an exchange's
 * items). One execution loads, for every message, i < n_lids and l < levels, the value from the
 * source field once and stores it to the buffer where a ghx_uplan pack of src writes it and to
 * the target cell a ghx_uplan unpack of dst writes: byte for byte what pack followed by unpack
 * leaves in the buffers and the fields, as ONE launch (k_self_u) that reads no buffer byte. Pad
 * bytes between entries are not written. Execution is stream-ordered, never allocates and can be
 * captured. The row decomposition is ghx_uput_create's, one per message for both sides (mode 0
 * only where the levels are contiguous on both); message row r sits at
 * buffer_offset + r * row_bytes in every mode; lists beyond 2^30 bytes split as theirs do; the
 * vector width is also narrowed by buffer_offset and, at launch, by buffer pointer + offset.
 * Messages of 4- or 8-byte rows move 16 bytes per lane (knob "urun") when every buffer pointer +
 * offset is 16-byte aligned and both field pointers are aligned to the row: the buffer side is
 * then one 16-byte store, each field side as in ghx_uput_create.
 * Created without a device like every other plan (execution then reports GHX_ERR_HIP).
 * GHX_ERR_INVALID, with the reason in ghx_last_error(), when: the two sides of a message differ
 * in n_lids, elem_size, levels or levels_first, or in buffer_slot or buffer_offset; two messages'
 * byte ranges overlap in one buffer; a lid is negative; elem_size < 1 or levels < 1; a field or
 * buffer slot is negative or >= 64 (one launch, no launch groups); a row is longer than 1 GiB;
 * a cell (field slot, lid) is both a source and a target of the plan; a target cell appears
 * twice. The last two are what makes a launch whose loads and stores have no order equal to the
 * two-launch exchange exactly; patterns always pass them (send lists hold inner cells, receive
 * lists distinct outer cells). Source lids may repeat. Two slots given the same pointer stay the
 * caller's contract. */
typedef struct ghx_uself ghx_uself;
int ghx_uself_create(const ghx_upack_entry* src, const ghx_upack_entry* dst, int32_t n, ghx_uself** out);
int ghx_uself_execute(const ghx_uself* p, void* const* field_ptrs, int32_t n_fields,
                      void* const* buffer_ptrs, int32_t n_buffers, ghx_stream stream);
/* message bytes per execution, segments, workgroup tiles */
int ghx_uself_info(const ghx_uself* p, uint64_t* bytes, int32_t* n_segments, int32_t* n_tiles);
/* Segment k of a plan of ghx_uself_create (host only): ghx_uput_segment_info's fields with the
 * same meaning, then the segment's place in its buffer: its first message row at buf_off of
 * buffer buf_slot (wlog2 is narrowed by buf_off as well). GHX_ERR_INVALID for k out of range. */
typedef struct ghx_uself_segment_info
{
    int64_t src_field_off, src_index_stride_b, src_level_stride_b;
    int64_t dst_field_off, dst_index_stride_b, dst_level_stride_b;
    int64_t first_index;
    uint32_t bytes;
    uint32_t row_bytes;
    uint32_t tile_bytes;
    uint32_t n;
    int32_t message;
    int32_t n_segments;                /* of the whole plan */
    int32_t src_slot, dst_slot;
    int32_t mode;
    int32_t wlog2;
    int32_t src_lid64, dst_lid64;
    int32_t src_runs, dst_runs;
    int32_t buf_slot;
    uint64_t buf_off;
} ghx_uself_segment_info;
int ghx_uself_segment(const ghx_uself* p, int32_t k, ghx_uself_segment_info* out);
int ghx_uself_destroy(ghx_uself* p);

/* The mixed form of the plan above: a pack of index-list messages that also completes those that
 * stay on the rank (no reference counterpart, as above). src[k] / dst[k], k < n_self, are the pack
 * and the unpack entry of one self message (ghx_uself_create's contract); peers[j], j < n_peers,
 * are pack entries of messages that leave the rank (pack only). The field slots of all three
 * arrays index ONE field pointer array, the buffer slots the send buffers. The result is an
 * ordinary ghx_uself: ghx_uself_execute runs ONE launch (k_pack_self_u) that does for the self
 * messages what ghx_uself_create's launch does and packs the peer messages as a ghx_uplan pack of
 * `peers` does — byte for byte what a ghx_uplan pack of every entry followed by a ghx_uplan unpack
 * of dst leaves in the buffers and the fields. ghx_uself_info reports bytes, segments and tiles of
 * both parts, ghx_uself_segment describes the self segments, ghx_umixed_peer_segment the peer
 * ones, ghx_uself_destroy frees it. The self part is exactly ghx_uself_create's plan (rows,
 * tiles, refusals); the peer part has exactly the segments and tiles of
 * ghx_uplan_create(peers, n_peers, 0): the same wlog2, mode, tiles and split below 2^30 bytes, in
 * one launch group. The launch takes the 16-byte run path (knob "urun") only when every segment of
 * both parts qualifies with the launch's pointers; a message moves the same bytes either way.
 * Created without a device. GHX_ERR_INVALID, with the reason in ghx_last_error(), for every
 * reason of ghx_uself_create and when: n_self < 1 or n_peers < 1 (an all-self plan is
 * ghx_uself_create's, an all-peer one ghx_uplan_create's); a field or buffer slot of a peer entry
 * is negative or >= 64; a peer entry's byte range overlaps another message's, self or peer, in
 * one buffer; a cell (field slot, lid) that a self message writes is a source cell of a peer
 * entry. The last is the hazard rule: the two-launch exchange loads every pack source before it
 * stores any unpack target, one launch orders nothing, so the check is what makes them equal;
 * patterns always pass it (send lists hold inner cells, receive lists outer cells). The same lid
 * on another field slot is another cell; cells are compared as (field slot, lid), so entries that
 * describe one field slot with different layouts stay the caller's contract, as two slots given
 * the same pointer do. */
int ghx_umixed_create(const ghx_upack_entry* src, const ghx_upack_entry* dst, int32_t n_self,
                      const ghx_upack_entry* peers, int32_t n_peers, ghx_uself** out);
/* workgroup tiles of the self part, segments and tiles of the peer part; a plan of
 * ghx_uself_create reports its tiles as self tiles and zeros for the peer part */
int ghx_umixed_info(const ghx_uself* p, int32_t* n_self_tiles, int32_t* n_peer_segments,
                    int32_t* n_peer_tiles);
/* Peer segment k of a plan of ghx_umixed_create (host only), as ghx_uplan_segment describes the
 * segments of the pack plan of `peers`. GHX_ERR_INVALID for k out of range or a plan without a
 * peer part. */
int ghx_umixed_peer_segment(const ghx_uself* p, int32_t k, ghx_usegment_info* out);

/* The fused self exchange of an exchange of unstructured items. ghx_exchange_create also plans
 * ONE launch (a ghx_uself over the exchange's pack and unpack entries, paired by buffer slot and
 * buffer offset) when the exchange has unstructured items only and at least one message, every
 * buffer of both directions belongs to this rank, recv buffer i is send buffer i (same domain
 * pair, same size), and ghx_uself_create's conditions hold (at most 64 items and 64 buffers among
 * them). ghx_uexchange_self_info works without a device; with *fusable = 0, ghx_last_error()
 * holds the reason. ghx_uexchange_self has ghx_exchange_self's argument contract (the buffers are
 * the send buffers, which hold the packed message afterwards) and fails with GHX_ERR_INVALID on
 * an exchange that is not fusable or whose send side has parity set (ghx_exchange_set_parity,
 * direction 0). ghx_exchange_self_fusable, ghx_exchange_mixed and ghx_cs_self_info are unchanged
 * by it: an exchange of unstructured items still reports 0 there. */
int ghx_uexchange_self_info(const ghx_exchange* ex, int32_t* fusable, int32_t* n_segments,
                            int32_t* n_tiles);
int ghx_uexchange_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                       void* const* buffers, int32_t n_buffers, ghx_stream stream);

/* The mixed form of an exchange of unstructured items with self AND peer messages — the index-list
 * counterpart of ghx_exchange_mixed / ghx_exchange_pack_self / ghx_exchange_unpack_peers; the
 * reference's own test geometry (unstructured_test_case.hpp: four domains over two ranks) is such
 * an exchange. ghx_exchange_create also plans it (a ghx_umixed_create plan and the unpack plan of
 * the peer recv buffers) when: the exchange has unstructured items only; at least one recv buffer
 * is a self message (it belongs to this rank and a send buffer of the same domain pair, size and
 * rank exists); at least one send buffer goes to, or one recv buffer comes from, another rank;
 * the self messages' unpack entries pair one to one with pack entries at the same (send buffer
 * slot, buffer offset); and ghx_umixed_create's conditions hold (at most 64 items and 64 send
 * buffers among them). ghx_uexchange_mixed_info works without a device; with *mixed = 0,
 * ghx_last_error() holds the reason. ghx_uexchange_pack_self has ghx_exchange_pack's argument
 * contract: ONE launch packs every send buffer and writes the self messages' halos.
 * ghx_uexchange_unpack_peers has ghx_exchange_unpack's: it unpacks the peer recv buffers only,
 * addressed by the caller's recv buffer indices, and enqueues nothing when the rank receives from
 * no peer. Together they leave byte for byte what ghx_exchange_pack + ghx_exchange_unpack leave
 * in fields and send buffers (a self message's recv buffer being its send buffer); pad bytes are
 * not written. Both fail with GHX_ERR_INVALID on an exchange that is not mixed, or while either
 * direction has parity set (ghx_exchange_set_parity): the direct exchange stays on its launches.
 * ghx_exchange_mixed, ghx_exchange_self_fusable, ghx_uexchange_self_info and ghx_cs_self_info are
 * unchanged by it. */
int ghx_uexchange_mixed_info(const ghx_exchange* ex, int32_t* mixed, int32_t* n_self_tiles,
                             int32_t* n_peer_tiles);
int ghx_uexchange_pack_self(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                            void* const* send_buffers, int32_t n_send, ghx_stream stream);
int ghx_uexchange_unpack_peers(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                               void* const* recv_buffers, int32_t n_recv, ghx_stream stream);

/* ------------------------------------------------------------------------------------------
 * Adjoint halo exchange of unstructured fields (no reference counterpart): the transpose of the
 * exchange. Message m of an exchange copies R[r_m[i], l] = S[s_m[i], l]; its adjoint does
 * S[s_m[i], l] += R[r_m[i], l] for every m, i and level l and then, with zero_halos, sets
 * R[r_m[i], l] to zero bytes: (owner, halo) -> (owner + sum of halos, 0). It runs as two launches
 * around the transport: a reverse pack (a ghx_uplan of direction 0 over the RECEIVE lists gathers
 * the halo cells into the receive buffers), and, once the bytes have travelled back into the SEND
 * buffers, the accumulate below (k_accum_u), the only kernel that knows an element type.
 * The sum is bitwise reproducible: no atomics; a destination cell starts from its own value and
 * adds its contributions one by one in ascending (contribution entry index, position in that
 * entry's list), in the element type, without reassociation. Integers wrap.
 * ------------------------------------------------------------------------------------------ */
#define GHX_DT_F32 1
#define GHX_DT_F64 2
#define GHX_DT_I32 3
#define GHX_DT_I64 4

/* The accumulate plan. contrib[e], e < n, are ghx_upack_entry as the pack entries of an exchange:
 * the field slot and lids of the OWNER side, the buffer slot and offset of the message, whose
 * bytes lie as ghx_udata_desc says ([i][level] with levels_first, else [level][i]); dtypes[e] is
 * the GHX_DT_* code of entry e's elements. zero[k], k < n_zero, name the HALO side (field slot and
 * lids; buffer members ignored). The planner builds, on the host and without a device: the
 * destination table (the distinct (field slot, lid) cells of contrib, sorted by slot then lid),
 * per destination a range of contribution records (entry, position) sorted by (entry, position),
 * one small record per entry, the distinct zero cells after the sum destinations, and one tile
 * table of "u_tile_rows" destination rows of one field slot per workgroup. One execution does,
 * for every sum destination and level, cell = (((cell + c0) + c1) + ...) over its records in
 * order, each c read from buffer_ptrs[buffer_slot]; with zero_halos != 0 it also stores zero bytes
 * to every zero cell (with zero_halos == 0 the launch leaves the trailing zero tiles out). One
 * launch, stream-ordered, never allocates, can be captured. Buffer ranges that overlap are
 * accepted: contributions are only read.
 * GHX_ERR_INVALID, with the reason in ghx_last_error(), when: a dtype code is unknown or its size
 * differs from the entry's elem_size; a zero entry's elem_size is not 4 or 8; levels < 1; a
 * field or buffer slot is negative or >= 64 (one launch, no launch groups); a list is null with
 * n_lids > 0, n_lids < 0 or a lid is negative; two entries of one field slot differ in their
 * descriptor or dtype; buffer_offset is no multiple of the element size; a cell is both a sum
 * destination and a zero destination; the plan would hold more than 2^32 - 1 contribution
 * records (or zero cells). Execution refuses pointers that are not aligned to the element. */
typedef struct ghx_uaccum ghx_uaccum;
int ghx_uaccum_create(const ghx_upack_entry* contrib, const int32_t* dtypes, int32_t n,
                      const ghx_upack_entry* zero, int32_t n_zero, ghx_uaccum** out);
int ghx_uaccum_execute(const ghx_uaccum* p, void* const* field_ptrs, int32_t n_fields,
                       void* const* buffer_ptrs, int32_t n_buffers, int32_t zero_halos,
                       ghx_stream stream);
/* buffer bytes read per execution, sum destinations, zero destinations, contribution records, the
 * most records of one destination, workgroup tiles (sum and zero tiles) */
int ghx_uaccum_info(const ghx_uaccum* p, uint64_t* bytes, int64_t* n_dest, int64_t* n_zero_dest,
                    int64_t* n_contrib, int64_t* max_per_dest, int32_t* n_tiles);
/* Destination k of the plan (host only, the twin of ghx_uself_segment), k in [0, n_dest +
 * n_zero_dest): its cell, and for a sum destination its records [first, first + count) of
 * ghx_uaccum_contrib; a zero destination has zero = 1 and no records. */
typedef struct ghx_uaccum_dest_info
{
    int32_t field_slot;
    int32_t zero;
    int64_t lid;
    int64_t first;
    int64_t count;
} ghx_uaccum_dest_info;
int ghx_uaccum_dest(const ghx_uaccum* p, int64_t k, ghx_uaccum_dest_info* out);
/* Contribution record j in [0, n_contrib): the contribution entry and the position in its list. */
int ghx_uaccum_contrib(const ghx_uaccum* p, int64_t j, int32_t* entry, int64_t* pos);
int ghx_uaccum_destroy(ghx_uaccum* p);

/* The get-accumulate (k_accum_get_u), the twin of ghx_saccum_get_create: ghx_uaccum_create's
 * operation, S[s_e[i], l] += R_e[i, l] in ascending (entry, position) per destination cell, where a
 * contribution entry may read R_e where it lies - the halo cells of a receiving field of the same
 * launch - instead of a buffer. source[e], e < n, is the halo side of contribution entry e's
 * message (field slot, descriptor and lids; buffer members ignored; position i pairs with position
 * i) or NULL: the entry reads its buffer as in ghx_uaccum_create. The array `source` itself is
 * required, also with n == 0 (a null array is refused). The two sides agree in n_lids,
 * levels and elem_size and may differ in index_stride, level_stride and levels_first. The
 * destination table, the ranges, the record order and the sum tiles are those of ghx_uaccum_create
 * on the same entries, so with the same halo values the sums are the same bit for bit; a record of
 * an entry with a source holds the source lid, resolved at plan time (records widen to 64-bit
 * lids, one table per plan, when a source lid is 2^31 or more). zero[k] as in ghx_uaccum_create,
 * but a zero entry that is a contribution's source (same field slot, same list) gets no zero
 * tiles: with zero_halos the lane that loaded a halo value stores zero bytes over it. That is
 * race-free because the planner verifies, and refuses otherwise, that every source cell is read by
 * one record and touched by nothing else. field_ptrs serve both sides; buffer_ptrs need cover only
 * the slots of entries without a source (their own buffer members are not looked at otherwise).
 * ghx_uaccum_info (bytes: the buffer bytes read) / _dest / _contrib / _destroy work on the plan;
 * ghx_uaccum_execute refuses it, as ghx_uaccum_get_execute refuses a plan of ghx_uaccum_create.
 * GHX_ERR_INVALID, with the reason, for ghx_uaccum_create's reasons (field slots of sources
 * included) and when: an entry and its source differ in n_lids, levels or elem_size; a source cell
 * (field slot, lid) is read by more than one record - a lid repeated within a receive list, or two
 * receive lists of one field slot naming the same cell; a source cell is also a sum destination;
 * a source cell lies in a zero entry that is no source. */
int ghx_uaccum_get_create(const ghx_upack_entry* contrib, const int32_t* dtypes,
                          const ghx_upack_entry* const* source, int32_t n,
                          const ghx_upack_entry* zero, int32_t n_zero, ghx_uaccum** out);
int ghx_uaccum_get_execute(const ghx_uaccum* p, void* const* field_ptrs, int32_t n_fields,
                           void* const* buffer_ptrs, int32_t n_buffers, int32_t zero_halos,
                           ghx_stream stream);
/* Contribution record j (host only, any plan): kind 0 = a buffer, 1 = a field source; the buffer
 * slot or the source field's slot; the source lid (-1 for a buffer record, whose position
 * ghx_uaccum_contrib gives). */
int ghx_uaccum_contrib_kind(const ghx_uaccum* p, int64_t j, int32_t* kind, int32_t* slot,
                            int64_t* lid);

/* The adjoint of an exchange of unstructured items. ghx_uexchange_adjoint_create builds and
 * attaches two plans (setup time, synchronous upload, as ghx_exchange_split attaches its plans):
 * the reverse pack, a ghx_uplan of direction 0 over the exchange's unpack entries, and the
 * accumulate plan with the exchange's pack entries as contribution entries and its unpack entries
 * as zero entries. dtypes[i] is the GHX_DT_* code of item i (n_items: the exchange's).
 * GHX_ERR_INVALID, with the reason, for an exchange that holds a structured or cubed-sphere item,
 * while a direction has parity set (ghx_exchange_set_parity), and for ghx_uaccum_create's
 * reasons. ghx_uexchange_adjoint_info works on any exchange: *ready = 1 once the plans exist.
 * ghx_uexchange_adjoint_pack has ghx_exchange_unpack's argument contract (it writes the RECEIVE
 * buffers), ghx_uexchange_adjoint_accumulate ghx_exchange_pack's (it reads the SEND buffers);
 * the caller moves the bytes of every receive buffer into the send buffer of the same message
 * between them (a self message's receive buffer is its send buffer). Both fail with
 * GHX_ERR_INVALID before create and while a direction has parity set. */
int ghx_uexchange_adjoint_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items);
int ghx_uexchange_adjoint_info(const ghx_exchange* ex, int32_t* ready, int64_t* n_dest,
                               int64_t* n_contrib);
int ghx_uexchange_adjoint_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                               void* const* recv_buffers, int32_t n_recv, ghx_stream stream);
int ghx_uexchange_adjoint_accumulate(const ghx_exchange* ex, void* const* field_ptrs,
                                     int32_t n_fields, void* const* send_buffers, int32_t n_send,
                                     int32_t zero_halos, ghx_stream stream);

/* The same adjoint with the self messages fused (k_accum_get_u), the twin of
 * ghx_sexchange_adjoint_self_*: a message whose receiver is a field of this rank (the pairing of
 * ghx_uexchange_pack_self: a receive buffer of this rank with a send buffer of the same pair of
 * domains and size) is accumulated straight from the receiving field's halo cells, and its buffer
 * is neither written nor read. self_create attaches a get plan (ghx_uaccum_get_create: every send
 * entry of a self message sourced by the receive entry at the same message bytes) and, where peer
 * messages remain, a reverse pack over the peer receive entries alone - those
 * ghx_uexchange_unpack_peers covers. It refuses what ghx_uexchange_adjoint_create refuses, an
 * exchange with no self message (ghx_uexchange_adjoint_create serves it), a self message whose two
 * sides do not pair, and ghx_uaccum_get_create's reasons (a halo cell of one self message that is
 * an owner cell of another message, for one); a refused create leaves every existing plan set as
 * it was, and the plans of ghx_uexchange_adjoint_create are independent of these. self_info works
 * on any exchange: form 0 = none, 1 = every message is a self message, 2 = mixed; sum
 * destinations, contribution records and how many contribution entries have a field source.
 * self_pack has ghx_uexchange_adjoint_pack's argument contract: form 1 launches nothing and
 * returns GHX_OK, form 2 gathers the peer messages' halo cells into their receive buffers.
 * self_accumulate has ghx_uexchange_adjoint_accumulate's: one k_accum_get_u launch, self messages
 * from the halos, peer messages from the send buffers. */
int ghx_uexchange_adjoint_self_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items);
int ghx_uexchange_adjoint_self_info(const ghx_exchange* ex, int32_t* form, int64_t* n_dest,
                                    int64_t* n_contrib, int64_t* n_field_sources);
int ghx_uexchange_adjoint_self_pack(const ghx_exchange* ex, void* const* field_ptrs,
                                    int32_t n_fields, void* const* recv_buffers, int32_t n_recv,
                                    ghx_stream stream);
int ghx_uexchange_adjoint_self_accumulate(const ghx_exchange* ex, void* const* field_ptrs,
                                          int32_t n_fields, void* const* send_buffers,
                                          int32_t n_send, int32_t zero_halos, ghx_stream stream);

/* ------------------------------------------------------------------------------------------
 * Adjoint halo exchange of structured fields (no reference counterpart): the operation above with
 * boxes in place of lists. Message m of an exchange pairs box k of a send entry with box k of the
 * peer's receive entry (equal extents) and copies R[recv cell] = S[send cell] cell by cell in
 * buffer order; its adjoint does S[send cell] += R[recv cell] for every message, box and cell
 * (component axis included) and then, with zero_halos, stores zero bytes to every receive-box
 * cell. Two launches around the transport: a reverse pack (a ghx_plan of direction 0 over the
 * RECEIVE entries) and the accumulate below (k_accum_s), which reads the SEND buffers.
 * A field's send boxes overlap (a corner cell of a periodic domain lies in 7 of them, every cell
 * of a domain narrower than its halo in up to 26). The planner cuts, per field slot, the union of
 * the contribution boxes into disjoint sub-boxes — every dimension at every box's first and
 * last + 1, elementary boxes no box holds dropped, neighbours along the fastest spatial dimension
 * with equal source lists merged — so every cell of a sub-box has the same sources: the boxes
 * that hold it, in ascending (entry, box). A destination cell starts from its own value and adds
 * its contributions one at a time in that order, in the element type, without reassociation or
 * contraction; integers as unsigned (they wrap). Bitwise reproducible, no atomics.
 *
 * contrib[e], e < n, are ghx_pack_entry as the pack entries of an exchange (the buffer position of
 * a box cell is the one ghx_plan_create gives it: boxes one after the other from buffer_offset,
 * each dense in layout order with the component axis); dtypes[e] the GHX_DT_* code of entry e.
 * zero[k] name the halo side (field slot, descriptor and boxes; buffer members ignored): their
 * boxes become zero sub-boxes without sources. Tiles: the rows of one sub-box (runs along the
 * layout's fastest dimension; single elements where that dimension is strided) cut by the
 * "tile_bytes" knob in field bytes, sum tiles first, so a launch without zero_halos runs those
 * only. One launch, stream-ordered, never allocates, can be captured.
 * GHX_ERR_INVALID, with the reason in ghx_last_error(), when: a dtype code is unknown or its size
 * differs from the entry's elem_size; a zero entry's elem_size is not 4 or 8; a field or buffer
 * slot is negative or >= 64 (one launch, no launch groups); two entries of one field slot differ
 * in their field descriptor or dtype; a byte stride of a field is no multiple of its element;
 * buffer_offset is no multiple of the element size; a cell is both summed and zeroed; a box lies
 * outside the field's extents (ghx_plan_create's rule) or has first > last; the plan would hold
 * more than 2^32 - 1 source records. Overlapping buffer ranges are accepted: contributions are
 * only read. Execution refuses pointer arrays that do not cover the plan's slots and pointers
 * that are not aligned to the element.
 * ------------------------------------------------------------------------------------------ */
typedef struct ghx_saccum ghx_saccum;
int ghx_saccum_create(const ghx_pack_entry* contrib, const int32_t* dtypes, int32_t n,
                      const ghx_pack_entry* zero, int32_t n_zero, ghx_saccum** out);
int ghx_saccum_execute(const ghx_saccum* p, void* const* field_ptrs, int32_t n_fields,
                       void* const* buffer_ptrs, int32_t n_buffers, int32_t zero_halos,
                       ghx_stream stream);
/* buffer bytes read per execution, sum sub-boxes, zero sub-boxes, source records, the longest
 * source list, workgroup tiles (sum and zero tiles) */
int ghx_saccum_info(const ghx_saccum* p, uint64_t* bytes, int64_t* n_boxes, int64_t* n_zero_boxes,
                    int64_t* n_sources, int64_t* max_sources, int32_t* n_tiles);
/* Sub-box k of the plan (host only), k in [0, n_boxes + n_zero_boxes): its bounds in the field's
 * local coordinates (spatial dims), the length of its rows in elements, the planned vector width
 * and, for a sum sub-box, its records [first_src, first_src + n_src) of ghx_saccum_source; a zero
 * sub-box has zero = 1 and no records. */
typedef struct ghx_saccum_box_info
{
    int32_t field_slot;
    int32_t zero;
    int32_t first[GHX_MAX_DIM];
    int32_t last[GHX_MAX_DIM];
    int64_t row_elems;
    int32_t wlog2;
    int32_t pad;
    int64_t first_src;
    int64_t n_src;
} ghx_saccum_box_info;
int ghx_saccum_box(const ghx_saccum* p, int64_t k, ghx_saccum_box_info* out);
/* Source record j in [0, n_sources): the contribution entry and its box, the buffer slot and the
 * byte offset in that buffer of the cell at the sub-box's origin (component 0). */
int ghx_saccum_source(const ghx_saccum* p, int64_t j, int32_t* entry, int32_t* box,
                      int32_t* buffer_slot, uint64_t* buffer_offset_of_origin);
int ghx_saccum_destroy(ghx_saccum* p);

/* The get-accumulate (k_accum_get_s): ghx_saccum_create's operation, S[send cell] += R[recv cell] in
 * ascending (entry, box), where a contribution entry may read R where it lies — the halo cells of a
 * receiving field of the same launch — instead of a buffer. source[e], e < n, is the halo side of
 * contribution entry e's message (field slot, descriptor and boxes; buffer members ignored; box k
 * pairs with box k) or NULL: the entry reads its buffer as in ghx_saccum_create. Source records
 * then hold the field byte offset of the sub-box's origin in the source field and that field's
 * byte strides; the cutting, the merging, the list order and the record layout stay (a sub-box
 * whose fastest dimension is strided in a source field takes single elements as rows). A sub-box's
 * list may mix both kinds. zero[k] as in ghx_saccum_create, but a zero entry that is a
 * contribution's source (same field slot, same boxes) gets no zero tiles: with zero_halos the lane
 * that loaded a halo vector stores zero bytes over it. That is race-free because the planner
 * verifies, and refuses otherwise, that every source cell is read by one (cell, source) pair and
 * touched by nothing else. ghx_saccum_execute's field_ptrs serve both sides; buffer_ptrs need cover
 * only the slots of entries without a source. ghx_saccum_info / _box / _source / _destroy work on
 * the plan (_source's buffer_slot is then the record's index in the launch's source pointer table:
 * the buffer slots that are read, ascending, then the source field slots, ascending);
 * ghx_saccum_execute refuses it, as ghx_saccum_get_execute refuses a plan of ghx_saccum_create.
 * GHX_ERR_INVALID, with the reason, for ghx_saccum_create's reasons and when: an entry and its
 * source differ in their number of boxes, in a box's extents, in elem_size, dimensions,
 * components or layout order; two source boxes of one field slot meet; a source box meets a
 * contribution box, or a zero box of an entry that is no source, of the same field slot; the source
 * pointer table would hold more than 64 slots. */
int ghx_saccum_get_create(const ghx_pack_entry* contrib, const int32_t* dtypes,
                          const ghx_pack_entry* const* source, int32_t n, const ghx_pack_entry* zero,
                          int32_t n_zero, ghx_saccum** out);
int ghx_saccum_get_execute(const ghx_saccum* p, void* const* field_ptrs, int32_t n_fields,
                           void* const* buffer_ptrs, int32_t n_buffers, int32_t zero_halos,
                           ghx_stream stream);
/* Source record j (host only, any plan): kind 0 = a buffer, 1 = a field source; the buffer slot or
 * the source field's slot; the byte offset there of the cell at the sub-box's origin. */
int ghx_saccum_source_kind(const ghx_saccum* p, int64_t j, int32_t* kind, int32_t* slot,
                           uint64_t* offset_of_origin);

/* The adjoint of an exchange of regular structured items, the twin of ghx_uexchange_adjoint_*:
 * create attaches the reverse pack (a ghx_plan of direction 0 over the exchange's unpack entries)
 * and the accumulate plan (pack entries as contribution entries, unpack entries as zero entries);
 * dtypes[i] is the GHX_DT_* code of item i. GHX_ERR_INVALID, with the reason, for an exchange that
 * holds an unstructured or a cubed-sphere item, while a direction has parity set, and for
 * ghx_saccum_create's reasons. info works on any exchange. pack has ghx_exchange_unpack's argument
 * contract (it writes the RECEIVE buffers), accumulate ghx_exchange_pack's (it reads the SEND
 * buffers); both fail with GHX_ERR_INVALID before create and while a direction has parity set. */
int ghx_sexchange_adjoint_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items);
int ghx_sexchange_adjoint_info(const ghx_exchange* ex, int32_t* ready, int64_t* n_boxes,
                               int64_t* n_sources);
int ghx_sexchange_adjoint_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                               void* const* recv_buffers, int32_t n_recv, ghx_stream stream);
int ghx_sexchange_adjoint_accumulate(const ghx_exchange* ex, void* const* field_ptrs,
                                     int32_t n_fields, void* const* send_buffers, int32_t n_send,
                                     int32_t zero_halos, ghx_stream stream);

/* The same adjoint with the self messages fused: a message whose receiver is a field of this rank
 * (the pairing of ghx_exchange_pack_self: a receive buffer of this rank with a send buffer of the
 * same pair of domains and size) is accumulated straight from the receiving field's halo cells, and
 * its buffer is neither written nor read. self_create attaches a get plan (ghx_saccum_get_create:
 * every send entry of a self message sourced by the receive entry at the same message bytes) and,
 * where peer messages remain, a reverse pack over the peer receive entries alone — those
 * ghx_exchange_unpack_peers covers. It refuses what ghx_sexchange_adjoint_create refuses, an
 * exchange with no self message, and a self message whose two sides do not pair; it leaves the
 * plans of ghx_sexchange_adjoint_create alone. self_info works on any exchange: form 0 = none,
 * 1 = every message is a self message, 2 = mixed; sum sub-boxes, source records and how many
 * contribution entries have a field source. self_pack has ghx_sexchange_adjoint_pack's argument
 * contract: form 1 launches nothing and returns GHX_OK, form 2 gathers the peer messages' halo
 * cells into their receive buffers. self_accumulate has ghx_sexchange_adjoint_accumulate's: one
 * k_accum_get_s launch, self messages from the halos, peer messages from the send buffers. */
int ghx_sexchange_adjoint_self_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items);
int ghx_sexchange_adjoint_self_info(const ghx_exchange* ex, int32_t* form, int64_t* n_boxes,
                                    int64_t* n_sources, int64_t* n_field_sources);
int ghx_sexchange_adjoint_self_pack(const ghx_exchange* ex, void* const* field_ptrs,
                                    int32_t n_fields, void* const* recv_buffers, int32_t n_recv,
                                    ghx_stream stream);
int ghx_sexchange_adjoint_self_accumulate(const ghx_exchange* ex, void* const* field_ptrs,
                                          int32_t n_fields, void* const* send_buffers,
                                          int32_t n_send, int32_t zero_halos, ghx_stream stream);

/* The adjoint of a cubed-sphere exchange (ghx_cs_exchange_create), the third twin. The forward
 * unpack sets R[x, y, z, k] = s_k * B[T(x, y), z, k] (B the dense box in the neighbour tile's
 * coordinates, s_k = -1 for the vector components the edge's transform negates); the transpose is
 *   1. the reverse pack  B[T(x, y), z, k] = s_k * R[x, y, z, k]  into the RECEIVE buffers: a pack
 *      launch over the exchange's ordinary receive segments, then k_pack_x over the transformed
 *      unpack's own tile records (no second table);
 *   2. after the transport with the roles swapped (a self message's receive buffer is its send
 *      buffer), S[send cell] += B[cell] for every send entry, box and cell in ascending (send
 *      entry, box): ghx_saccum_create's plan over the exchange's send entries (the send side of a
 *      cubed-sphere exchange is ordinary boxes of the sender's field), bitwise reproducible, no
 *      atomics; with zero_halos zero bytes are then stored into every receive box. Halo cells no
 *      receive box holds (the cube-corner squares) keep their values.
 * dtypes[i] is the GHX_DT_* code of item i. create: GHX_ERR_INVALID, with the reason, for an
 * exchange that is not a cubed-sphere exchange, while a direction has parity set, when n_items is
 * not the exchange's or a code is unknown, when a code's size differs from the item's elem_size,
 * when a vector item's value_kind disagrees with its code (1: F32 / F64, 2: I32 / I64), and for
 * ghx_saccum_create's reasons (more than 64 field or buffer slots among them: a whole 24-domain
 * cube on one rank has 168 buffers; split it over ranks). info works on any exchange and without a
 * device: the sum sub-boxes and source records of the accumulate plan, and the records (spaces)
 * and tiles k_pack_x runs (ghx_cs_plan_info's). plan lends the accumulate plan (owned by the
 * exchange) to ghx_saccum_info / _box / _source. pack has ghx_exchange_unpack's argument contract
 * (it writes the RECEIVE buffers), accumulate ghx_exchange_pack's (it reads the SEND buffers);
 * both fail with GHX_ERR_INVALID before create and while a direction has parity set, allocate
 * nothing and can be captured in a graph. ghx_sexchange_adjoint_create and
 * ghx_uexchange_adjoint_create refuse a cubed-sphere exchange as before. */
int ghx_cs_exchange_adjoint_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items);
int ghx_cs_exchange_adjoint_info(const ghx_exchange* ex, int32_t* ready, int64_t* n_boxes,
                                 int64_t* n_sources, int32_t* n_pack_x_records,
                                 int32_t* n_pack_x_tiles);
int ghx_cs_exchange_adjoint_plan(const ghx_exchange* ex, const ghx_saccum** out);
/* The ordinary part of the reverse pack next to the ordinary part of the unpack it transposes:
 * their segment counts (equal once created; 0 before create / on any other exchange). */
int ghx_cs_exchange_adjoint_segments(const ghx_exchange* ex, int32_t* n_pack_segments,
                                     int32_t* n_unpack_segments);
int ghx_cs_exchange_adjoint_pack(const ghx_exchange* ex, void* const* field_ptrs, int32_t n_fields,
                                 void* const* recv_buffers, int32_t n_recv, ghx_stream stream);
int ghx_cs_exchange_adjoint_accumulate(const ghx_exchange* ex, void* const* field_ptrs,
                                       int32_t n_fields, void* const* send_buffers, int32_t n_send,
                                       int32_t zero_halos, ghx_stream stream);

/* The cubed-sphere adjoint with the self messages fused (k_accum_get_x), the twin of
 * ghx_sexchange_adjoint_self_*. A message whose receiver is a field of this rank is accumulated
 * straight from that field's halo cells: for every send entry, box and cell, in ascending (send
 * entry, box), S[cell] += s_k * R[T^-1(cell)] in the element type, R the receiving field of the same
 * message, T the edge's transform, s_k = -1 for the components it negates (a sign-bit flip for
 * floats, two's complement for integers, applied to the loaded value before the add: the bits are
 * those of ghx_cs_exchange_adjoint_pack + _accumulate). With zero_halos the lane that loaded a halo
 * value stores zero bytes over it. The buffers of self messages are neither written nor read, and
 * no buffer slot is spent on them: a whole 24-domain cube on one rank has an adjoint here with up
 * to two fields per domain (at most 64 field slots and 64 source-table slots, one launch).
 * self_create attaches the get plan — every send entry of a self message sourced by the receive
 * entry at the same message bytes, box k by box k, each box addressed through its space's transform
 * — and, where peer messages remain, the reverse pack of the peer receive spaces alone (the kept
 * ordinary segments and the transformed boxes, filtered by receive buffer). It refuses what
 * ghx_cs_exchange_adjoint_create refuses except that call's buffer-slot count, an exchange with no
 * self message, a self message whose two sides do not pair (element size, components, layout
 * order, number of boxes, shape under the transform), and ghx_saccum_get_create's reasons; it
 * leaves the plans of ghx_cs_exchange_adjoint_create alone. self_info works on any exchange and
 * without a device: form 0 = none, 1 = every message is a self message, 2 = mixed; sum sub-boxes,
 * source records, the contribution entries with a field source, and the paired boxes whose source
 * is transposed, reversed or signed. self_plan lends the plan (owned by the exchange) to
 * ghx_saccum_info / _box / _source / _source_kind / _source_map. self_segments: the ordinary
 * segments and the k_pack_x records (spaces) of form 2's reverse pack (0 in form 1 and before
 * create). ghx_saccum_source_map (host only, any plan): source record j's signed byte stride per
 * dimension of the contribution's field (strides[GHX_MAX_DIM]; a buffer source: its dense box's),
 * the components it negates (bit k: component k) and the component dimension (-1: none); with
 * ghx_saccum_source_kind's origin, cell (i_d) of a sub-box reads origin + sum (i_d - first_d) *
 * strides[d]. self_pack has ghx_cs_exchange_adjoint_pack's argument contract: form 1 launches
 * nothing, form 2 gathers the peer messages' halo cells. self_accumulate has
 * ghx_cs_exchange_adjoint_accumulate's: one k_accum_get_x launch, self messages from the halos,
 * peer messages from the send buffers; receive entries of peer messages get zero tiles. Both fail
 * with GHX_ERR_INVALID before self_create and while a direction has parity set, allocate nothing
 * and can be captured in a graph. */
int ghx_cs_exchange_adjoint_self_create(ghx_exchange* ex, const int32_t* dtypes, int32_t n_items);
int ghx_cs_exchange_adjoint_self_info(const ghx_exchange* ex, int32_t* form, int64_t* n_boxes,
                                      int64_t* n_sources, int64_t* n_field_sources,
                                      int64_t* n_rotated_sources);
int ghx_cs_exchange_adjoint_self_plan(const ghx_exchange* ex, const ghx_saccum** out);
int ghx_cs_exchange_adjoint_self_segments(const ghx_exchange* ex, int32_t* n_pack_segments,
                                          int32_t* n_pack_x_records);
int ghx_saccum_source_map(const ghx_saccum* p, int64_t j, int64_t* strides, int32_t* neg_mask,
                          int32_t* comp_dim);
int ghx_cs_exchange_adjoint_self_pack(const ghx_exchange* ex, void* const* field_ptrs,
                                      int32_t n_fields, void* const* recv_buffers, int32_t n_recv,
                                      ghx_stream stream);
int ghx_cs_exchange_adjoint_self_accumulate(const ghx_exchange* ex, void* const* field_ptrs,
                                            int32_t n_fields, void* const* send_buffers,
                                            int32_t n_send, int32_t zero_halos, ghx_stream stream);

/* Device-side access epochs of the zero-copy exchanges (bulk puts, direct pack): the reference's
 * access guards (include/ghex/rma/access_guard.hpp:35-140; per range: start/end_target_epoch on
 * the owner, start/end_source_epoch on the putter; include/ghex/bulk_communication_object.hpp
 * :621-694) as TWO stream-ordered launches around the data launch(es) — phase 0 (open) before,
 * phase 1 (close) after. The flags live in each rank's inbox, fine-grained device memory on its
 * GPU that its node-local peers map through IPC and write into, polled locally; a block of
 * node-shared host memory (POSIX shm `name`, "/...") carries the inbox handles and each rank's
 * epoch and error for the host (the creating rank passes create = 1 before the others attach
 * with 0, and one rank unlinks the name once all have attached). `world` and `rank` are the node-local group's size
 * and this rank's index in it (one block per host; at most 64 ranks per host). ghx_epochs_peers
 * (before the first ghx_epochs_enqueue; refused afterwards: enqueued kernels hold the peers'
 * inbox mappings) sets this rank's sources (ranks that write into its memory) and targets (ranks whose memory it
 * writes into) as node-local indices, excluding itself. Open: this rank's halos / receive
 * buffers are open to its sources; wait until each target has opened. Close: system-scope
 * release on every XCD (the grid is sized from the queried XCD count; the leader checks that
 * every XCD ran), signal each target, wait for each source, system-scope acquire on every XCD.
 * No host synchronisation, no barrier; the epoch counter lives in memory, so the sequence can
 * be captured into a graph. Waits are bounded: ghx_epochs_status reports 0, 1 / 2 (a wait of
 * the open / close phase timed out), 3 (the close kernel did not reach every XCD in time) or
 * 4 | s << 8 (source s failed an epoch wait: its later writes may have overlapped this rank's
 * reads). After a nonzero status the object is broken (every later wait returns at once). */
typedef struct ghx_epochs ghx_epochs;
int ghx_epochs_create(const char* name, int32_t create, int32_t world, int32_t rank,
                      double timeout_s, ghx_epochs** out);
int ghx_epochs_unlink(const char* name);
int ghx_epochs_peers(ghx_epochs* ep, const int32_t* sources, int32_t n_sources,
                     const int32_t* targets, int32_t n_targets);
int ghx_epochs_enqueue(ghx_epochs* ep, int32_t phase, ghx_stream stream);
int ghx_epochs_status(const ghx_epochs* ep, int32_t* error, uint64_t* epoch);
int ghx_epochs_info(const ghx_epochs* ep, int32_t* n_xcc, int32_t* fence_groups);
/* Phase 2 (one launch per exchange) is for receive memory double-buffered by epoch parity
 * (ghx_exchange_set_parity with the word ghx_epochs_counter returns): data launch (copy e&1 of
 * the targets') -> ghx_epochs_enqueue(ep, 2, stream) -> unpack (copy e&1 of this rank's). The
 * close tells the sources that this rank's previous unpack is done, which is what the open
 * phase is for otherwise. An object runs phases 0/1 or phase 2, not both. Without peers the
 * close phases enqueue nothing. */
int ghx_epochs_counter(const ghx_epochs* ep, const uint64_t** word);
int ghx_epochs_destroy(ghx_epochs* ep);

/* ------------------------------------------------------------------------------------------
 * Host staging copies (the NIC-side path): device <-> pinned host copies on
 * SDMA engines chosen by measurement. Replaces the staging the reference leaves to its transport
 * (oomph device/host buffers, include/ghex/arch_traits.hpp:51-75; the non-stream-aware branch of
 * include/ghex/communication_object.hpp:611-637, 715-729). hipMemcpyAsync lets the runtime pick
 * the engine, and D2H and H2D of one exchange often end up on one engine (serialised) or on a
 * slow one; ghx_copier_create probes engines 0-3 with `probe_bytes` copies per direction and
 * alone / concurrently, and keeps the pair (D2H engine, H2D engine) with the best concurrent
 * rate (ghx_copier_info). ghx_copier_submit enqueues one copy (direction 0 = device -> host,
 * 1 = host -> device; host memory must be pinned, e.g. hipHostMalloc) and returns a ticket; with
 * after_ticket >= 0 the copy engine starts it only once that earlier copy has completed (no host
 * round trip). ghx_copier_wait blocks until a ticket's copy has completed (error after
 * `timeout_s`). ghx_copier_acquire enqueues, on a stream, the cache invalidation that kernels
 * reading bytes an H2D copy has written need before them (the HIP runtime does not see these
 * copies, so it would not add it). Not thread-safe: one copier per thread. */
typedef struct ghx_copier ghx_copier;
int ghx_copier_create(uint64_t probe_bytes, double timeout_s, ghx_copier** out);
int ghx_copier_info(const ghx_copier* c, int32_t* d2h_engine, int32_t* h2d_engine, float* d2h_GBps,
                    float* h2d_GBps, float* both_GBps);
int ghx_copier_submit(ghx_copier* c, void* dst, const void* src, uint64_t bytes, int32_t direction,
                      int64_t after_ticket, uint64_t* ticket);
int ghx_copier_wait(ghx_copier* c, uint64_t ticket);
int ghx_copier_acquire(const ghx_copier* c, ghx_stream stream);
int ghx_copier_destroy(ghx_copier* c);

#ifdef __cplusplus
}
#endif

#endif /* GHX_H */
