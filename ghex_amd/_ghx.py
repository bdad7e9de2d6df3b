"""ctypes binding of libghx.so (include/ghx.h). Fails loudly when the library is missing:
there is no CPU fallback anywhere in ghex_amd."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libghx.so")

MAX_DIM = 4
MAX_SLOTS = 64

c_i32, c_i64, c_u64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p


class FieldDesc(ctypes.Structure):
    _fields_ = [("dim", c_i32), ("elem_size", c_i32), ("layout", c_i32 * MAX_DIM),
                ("byte_strides", c_i64 * MAX_DIM), ("offsets", c_i32 * MAX_DIM),
                ("extents", c_i32 * MAX_DIM), ("num_components", c_i32),
                ("has_components", c_i32)]


class Box(ctypes.Structure):
    _fields_ = [("first", c_i32 * MAX_DIM), ("last", c_i32 * MAX_DIM)]


class PackEntry(ctypes.Structure):
    _fields_ = [("field", FieldDesc), ("field_slot", c_i32), ("buffer_slot", c_i32),
                ("buffer_offset", c_u64), ("boxes", ctypes.POINTER(Box)), ("n_boxes", c_i32)]


class SegmentInfo(ctypes.Structure):
    _fields_ = [("field_off", c_i64), ("buf_off", c_u64), ("stride", c_i64 * 4),
                ("ext", ctypes.c_uint32 * 4), ("row_bytes", ctypes.c_uint32),
                ("bytes", ctypes.c_uint32), ("tile_bytes", ctypes.c_uint32),
                ("field_slot", c_i32), ("buffer_slot", c_i32), ("n_outer", c_i32),
                ("wlog2", c_i32), ("amode", c_i32), ("pipe", c_i32)]


class UDataDesc(ctypes.Structure):
    _fields_ = [("elem_size", c_i32), ("levels", c_i32), ("levels_first", c_i32),
                ("index_stride", c_i64), ("level_stride", c_i64)]


class UPackEntry(ctypes.Structure):
    _fields_ = [("data", UDataDesc), ("field_slot", c_i32), ("buffer_slot", c_i32),
                ("buffer_offset", c_u64), ("lids", ctypes.POINTER(c_i64)), ("n_lids", c_i64)]


class USegmentInfo(ctypes.Structure):
    _fields_ = [("field_off", c_i64), ("buf_off", c_u64), ("index_stride_b", c_i64),
                ("level_stride_b", c_i64), ("bytes", ctypes.c_uint32),
                ("row_bytes", ctypes.c_uint32), ("tile_bytes", ctypes.c_uint32),
                ("n", ctypes.c_uint32), ("field_slot", c_i32), ("buffer_slot", c_i32),
                ("mode", c_i32), ("wlog2", c_i32), ("lid64", c_i32), ("runs", c_i32),
                ("fpol", c_i32)]


class UPutEntry(ctypes.Structure):
    _fields_ = [("data", UDataDesc), ("field_slot", c_i32), ("lids", ctypes.POINTER(c_i64)),
                ("n_lids", c_i64)]


class UPutSegmentInfo(ctypes.Structure):
    _fields_ = [("src_field_off", c_i64), ("src_index_stride_b", c_i64),
                ("src_level_stride_b", c_i64), ("dst_field_off", c_i64),
                ("dst_index_stride_b", c_i64), ("dst_level_stride_b", c_i64),
                ("first_index", c_i64), ("bytes", ctypes.c_uint32),
                ("row_bytes", ctypes.c_uint32), ("tile_bytes", ctypes.c_uint32),
                ("n", ctypes.c_uint32), ("message", c_i32), ("n_segments", c_i32),
                ("src_slot", c_i32), ("dst_slot", c_i32), ("mode", c_i32), ("wlog2", c_i32),
                ("src_lid64", c_i32), ("dst_lid64", c_i32), ("src_runs", c_i32),
                ("dst_runs", c_i32)]


class USelfSegmentInfo(ctypes.Structure):
    _fields_ = UPutSegmentInfo._fields_ + [("buf_slot", c_i32), ("buf_off", c_u64)]


class UAccumDestInfo(ctypes.Structure):
    _fields_ = [("field_slot", c_i32), ("zero", c_i32), ("lid", c_i64), ("first", c_i64),
                ("count", c_i64)]


class SAccumBoxInfo(ctypes.Structure):
    _fields_ = [("field_slot", c_i32), ("zero", c_i32), ("first", c_i32 * MAX_DIM),
                ("last", c_i32 * MAX_DIM), ("row_elems", c_i64), ("wlog2", c_i32), ("pad", c_i32),
                ("first_src", c_i64), ("n_src", c_i64)]


# element type codes of the adjoint accumulate (GHX_DT_*, include/ghx.h)
DT_F32, DT_F64, DT_I32, DT_I64 = 1, 2, 3, 4


class RegularDomain(ctypes.Structure):
    _fields_ = [("id", c_i32), ("rank", c_i32), ("first", c_i32 * 3), ("last", c_i32 * 3)]


class CsDomain(ctypes.Structure):
    _fields_ = [("rank", c_i32), ("tile", c_i32), ("x_first", c_i32), ("x_last", c_i32),
                ("y_first", c_i32), ("y_last", c_i32)]


class CsItem(ctypes.Structure):
    _fields_ = [("tile", c_i32), ("first_x", c_i32), ("first_y", c_i32), ("edge_size", c_i32),
                ("is_vector", c_i32), ("value_kind", c_i32)]


class ExchangeItem(ctypes.Structure):
    _fields_ = [("pattern", c_vp), ("local_index", c_i32), ("kind", c_i32), ("field", FieldDesc),
                ("udata", UDataDesc), ("align", c_i32), ("tag_offset", c_i32)]


P = ctypes.POINTER
_SIGS = {
    "ghx_tune": (c_i32, [ctypes.c_char_p, c_i32]),
    "ghx_launch_timing": (c_i32, [c_i32]),
    "ghx_launch_timing_read": (c_i32, [ctypes.POINTER(ctypes.c_float), c_i32,
                                       ctypes.POINTER(c_i32)]),
    "ghx_last_error": (ctypes.c_char_p, []),
    "ghx_version": (ctypes.c_char_p, []),
    "ghx_plan_create": (c_i32, [P(PackEntry), c_i32, c_i32, P(c_vp)]),
    "ghx_plan_execute": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_plan_destroy": (c_i32, [c_vp]),
    "ghx_plan_info": (c_i32, [c_vp, P(c_u64), P(c_i32), P(c_i32)]),
    "ghx_plan_segment": (c_i32, [c_vp, c_i32, P(SegmentInfo)]),
    "ghx_structured_pack": (c_i32, [P(FieldDesc), c_vp, c_vp, P(Box), c_i32, c_vp]),
    "ghx_structured_unpack": (c_i32, [P(FieldDesc), c_vp, c_vp, P(Box), c_i32, c_vp]),
    "ghx_uplan_create": (c_i32, [P(UPackEntry), c_i32, c_i32, P(c_vp)]),
    "ghx_uplan_execute": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_uplan_destroy": (c_i32, [c_vp]),
    "ghx_uplan_info": (c_i32, [c_vp, P(c_u64), P(c_i32), P(c_i32)]),
    "ghx_uplan_segment": (c_i32, [c_vp, c_i32, P(USegmentInfo)]),
    "ghx_regular_halo_boxes": (c_i32, [c_i32, P(c_i32), P(c_i32), P(c_i32), P(c_i32), P(c_i32),
                                       P(c_i32), P(Box), P(Box), c_i32, P(c_i32)]),
    "ghx_regular_pattern_create": (c_i32, [c_i32, P(RegularDomain), c_i32, P(c_i32), P(c_i32),
                                           P(c_i32), P(c_i32), c_i32, P(c_vp)]),
    "ghx_staged_pattern_create": (c_i32, [c_i32, P(RegularDomain), c_i32, P(c_i32), P(c_i32),
                                          P(c_i32), P(c_i32), P(c_i32), c_i32, P(c_vp)]),
    "ghx_cs_halo_boxes": (c_i32, [c_i32, c_i32, P(CsDomain), P(c_i32), P(Box), P(Box), P(c_i32),
                                  c_i32, P(c_i32)]),
    "ghx_cs_pattern_create": (c_i32, [c_i32, c_i32, P(CsDomain), c_i32, P(c_i32), c_i32,
                                      P(c_vp)]),
    "ghx_pattern_key_tiles": (c_i32, [c_vp, c_i32, c_i32, c_i32, P(c_i32), c_i32]),
    "ghx_cs_exchange_create": (c_i32, [P(ExchangeItem), P(CsItem), c_i32, P(c_vp)]),
    "ghx_cs_plan_info": (c_i32, [c_vp, P(c_i32), P(c_u64), P(c_i32), P(c_i32)]),
    "ghx_cs_self_info": (c_i32, [c_vp, P(c_i32), P(c_i32), P(c_i32), P(c_i32)]),
    "ghx_cs_exchange_self": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_uself_create": (c_i32, [P(UPackEntry), P(UPackEntry), c_i32, P(c_vp)]),
    "ghx_uself_execute": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_uself_info": (c_i32, [c_vp, P(c_u64), P(c_i32), P(c_i32)]),
    "ghx_uself_segment": (c_i32, [c_vp, c_i32, P(USelfSegmentInfo)]),
    "ghx_uself_destroy": (c_i32, [c_vp]),
    "ghx_uexchange_self_info": (c_i32, [c_vp, P(c_i32), P(c_i32), P(c_i32)]),
    "ghx_uexchange_self": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_umixed_create": (c_i32, [P(UPackEntry), P(UPackEntry), c_i32, P(UPackEntry), c_i32, P(c_vp)]),
    "ghx_umixed_info": (c_i32, [c_vp, P(c_i32), P(c_i32), P(c_i32)]),
    "ghx_umixed_peer_segment": (c_i32, [c_vp, c_i32, P(USegmentInfo)]),
    "ghx_uexchange_mixed_info": (c_i32, [c_vp, P(c_i32), P(c_i32), P(c_i32)]),
    "ghx_uexchange_pack_self": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_uexchange_unpack_peers": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_uaccum_create": (c_i32, [P(UPackEntry), P(c_i32), c_i32, P(UPackEntry), c_i32, P(c_vp)]),
    "ghx_uaccum_execute": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_i32, c_vp]),
    "ghx_uaccum_info": (c_i32, [c_vp, P(c_u64), P(c_i64), P(c_i64), P(c_i64), P(c_i64), P(c_i32)]),
    "ghx_uaccum_dest": (c_i32, [c_vp, c_i64, P(UAccumDestInfo)]),
    "ghx_uaccum_contrib": (c_i32, [c_vp, c_i64, P(c_i32), P(c_i64)]),
    "ghx_uaccum_destroy": (c_i32, [c_vp]),
    "ghx_uexchange_adjoint_info": (c_i32, [c_vp, P(c_i32), P(c_i64), P(c_i64)]),
    "ghx_uaccum_get_create": (c_i32, [P(UPackEntry), P(c_i32), P(P(UPackEntry)), c_i32, P(UPackEntry), c_i32,
                                      P(c_vp)]),
    "ghx_uaccum_get_execute": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_i32, c_vp]),
    "ghx_uaccum_contrib_kind": (c_i32, [c_vp, c_i64, P(c_i32), P(c_i32), P(c_i64)]),
    "ghx_uexchange_adjoint_self_info": (c_i32, [c_vp, P(c_i32), P(c_i64), P(c_i64), P(c_i64)]),
    "ghx_saccum_create": (c_i32, [P(PackEntry), P(c_i32), c_i32, P(PackEntry), c_i32, P(c_vp)]),
    "ghx_saccum_execute": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_i32, c_vp]),
    "ghx_saccum_info": (c_i32, [c_vp, P(c_u64), P(c_i64), P(c_i64), P(c_i64), P(c_i64), P(c_i32)]),
    "ghx_saccum_box": (c_i32, [c_vp, c_i64, P(SAccumBoxInfo)]),
    "ghx_saccum_source": (c_i32, [c_vp, c_i64, P(c_i32), P(c_i32), P(c_i32), P(c_u64)]),
    "ghx_saccum_destroy": (c_i32, [c_vp]),
    "ghx_saccum_get_create": (c_i32, [P(PackEntry), P(c_i32), P(P(PackEntry)), c_i32, P(PackEntry), c_i32, P(c_vp)]),
    "ghx_saccum_get_execute": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_i32, c_vp]),
    "ghx_saccum_source_kind": (c_i32, [c_vp, c_i64, P(c_i32), P(c_i32), P(c_u64)]),
    "ghx_sexchange_adjoint_self_info": (c_i32, [c_vp, P(c_i32), P(c_i64), P(c_i64), P(c_i64)]),
    "ghx_sexchange_adjoint_info": (c_i32, [c_vp, P(c_i32), P(c_i64), P(c_i64)]),
    "ghx_cs_exchange_adjoint_info": (c_i32, [c_vp, P(c_i32), P(c_i64), P(c_i64), P(c_i32), P(c_i32)]),
    "ghx_cs_exchange_adjoint_plan": (c_i32, [c_vp, P(c_vp)]),
    "ghx_cs_exchange_adjoint_segments": (c_i32, [c_vp, P(c_i32), P(c_i32)]),
    "ghx_cs_exchange_adjoint_self_info": (c_i32, [c_vp, P(c_i32), P(c_i64), P(c_i64), P(c_i64), P(c_i64)]),
    "ghx_cs_exchange_adjoint_self_plan": (c_i32, [c_vp, P(c_vp)]),
    "ghx_cs_exchange_adjoint_self_segments": (c_i32, [c_vp, P(c_i32), P(c_i32)]),
    "ghx_saccum_source_map": (c_i32, [c_vp, c_i64, P(c_i64), P(c_i32), P(c_i32)]),
    "ghx_cs_unpack": (c_i32, [P(FieldDesc), P(CsItem), c_vp, c_vp, P(Box), P(Box), P(c_i32),
                              c_i32, c_vp]),
    "ghx_cs_pack_rotated": (c_i32, [P(FieldDesc), P(CsItem), c_vp, c_vp, P(Box), P(Box), P(c_i32),
                                    c_i32, c_vp]),
    "ghx_udomain_create": (c_i32, [c_i32, P(c_i64), c_i64, P(c_i64), c_i64, P(c_vp)]),
    "ghx_udomain_destroy": (c_i32, [c_vp]),
    "ghx_udomain_info": (c_i32, [c_vp, P(c_i32), P(c_i64), P(c_i64), P(c_i64)]),
    "ghx_udomain_halo": (c_i32, [c_vp, P(c_i64), c_i64, P(c_i64), c_i64, P(c_i64)]),
    "ghx_upattern_create": (c_i32, [P(c_vp), c_i32, c_i32, c_i32, c_i32, P(c_vp)]),
    "ghx_upattern_add_halos": (c_i32, [c_vp, c_i32, c_i32, P(c_i32), P(c_i64), P(c_i64),
                                       P(c_i64)]),
    "ghx_upattern_record": (c_i32, [c_vp, c_i64, P(c_i32), P(c_i32), P(c_i32), P(c_i32),
                                    P(c_i64), P(P(c_i64))]),
    "ghx_upattern_add_recv": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, P(c_i64), c_i64]),
    "ghx_upattern_finish": (c_i32, [c_vp, P(c_vp)]),
    "ghx_upattern_destroy": (c_i32, [c_vp]),
    "ghx_pattern_destroy": (c_i32, [c_vp]),
    "ghx_pattern_filter": (c_i32, [c_vp, P(c_i32), c_i32, c_i32, P(c_vp)]),
    "ghx_pattern_num_domains": (c_i32, [c_vp, P(c_i32)]),
    "ghx_pattern_max_tag": (c_i32, [c_vp, P(c_i32)]),
    "ghx_pattern_domain_id": (c_i32, [c_vp, c_i32, P(c_i32)]),
    "ghx_pattern_num_keys": (c_i32, [c_vp, c_i32, c_i32, P(c_i32)]),
    "ghx_pattern_key": (c_i32, [c_vp, c_i32, c_i32, c_i32, P(c_i32), P(c_i32), P(c_i32),
                                P(c_i32), P(c_i64)]),
    "ghx_pattern_key_boxes": (c_i32, [c_vp, c_i32, c_i32, c_i32, P(Box), P(Box), c_i32]),
    "ghx_pattern_key_lids": (c_i32, [c_vp, c_i32, c_i32, c_i32, P(c_i64), c_i64]),
    "ghx_exchange_create": (c_i32, [P(ExchangeItem), c_i32, P(c_vp)]),
    "ghx_exchange_destroy": (c_i32, [c_vp]),
    "ghx_exchange_num_buffers": (c_i32, [c_vp, c_i32, P(c_i32)]),
    "ghx_exchange_buffer": (c_i32, [c_vp, c_i32, c_i32, P(c_i32), P(c_i32), P(c_i32), P(c_i32),
                                    P(c_u64)]),
    "ghx_exchange_pack": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_exchange_unpack": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_exchange_self_fusable": (c_i32, [c_vp, P(c_i32)]),
    "ghx_exchange_self": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_exchange_mixed": (c_i32, [c_vp, P(c_i32)]),
    "ghx_exchange_pack_self": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_exchange_unpack_peers": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_exchange_split": (c_i32, [c_vp]),
    "ghx_exchange_pack_buffer": (c_i32, [c_vp, c_i32, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_exchange_unpack_buffer": (c_i32, [c_vp, c_i32, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_rccl_open": (c_i32, [ctypes.c_char_p]),
    "ghx_rccl_unique_id": (c_i32, [P(ctypes.c_ubyte)]),
    "ghx_rccl_comm_init": (c_i32, [P(ctypes.c_ubyte), c_i32, c_i32, P(c_vp)]),
    "ghx_rccl_comm_destroy": (c_i32, [c_vp]),
    "ghx_rccl_comm_check": (c_i32, [c_vp]),
    "ghx_pipeline_create": (c_i32, [c_vp, c_i32, c_i32, P(c_i32), P(c_vp), P(c_i32), c_i32,
                                    P(c_vp)]),
    "ghx_pipeline_run": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_pipeline_destroy": (c_i32, [c_vp]),
    "ghx_unstructured_pack": (c_i32, [P(UDataDesc), c_vp, c_vp, c_vp, c_i32, ctypes.c_int64, c_vp]),
    "ghx_unstructured_unpack": (c_i32, [P(UDataDesc), c_vp, c_vp, c_vp, c_i32, ctypes.c_int64, c_vp]),
    "ghx_ipc_export": (c_i32, [c_vp, P(ctypes.c_ubyte), P(ctypes.c_uint64)]),
    "ghx_ipc_import": (c_i32, [P(ctypes.c_ubyte), ctypes.c_uint64, P(c_vp), P(c_vp)]),
    "ghx_ipc_close": (c_i32, [c_vp]),
    "ghx_put_create": (c_i32, [P(PackEntry), c_i32, P(PackEntry), c_i32, P(c_vp)]),
    "ghx_put_execute": (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp]),
    "ghx_put_info": (c_i32, [c_vp, P(ctypes.c_uint64), P(c_i32)]),
    "ghx_put_destroy": (c_i32, [c_vp]),
    "ghx_cs_put_create": (c_i32, [P(PackEntry), c_i32, P(PackEntry), c_i32, P(CsItem),
                                  P(P(Box)), P(P(c_i32)), P(c_vp)]),
    "ghx_cs_put_info": (c_i32, [c_vp, P(c_i32), P(c_i32), P(c_i32)]),
    "ghx_uput_create": (c_i32, [P(UPutEntry), P(UPutEntry), c_i32, P(c_vp)]),
    "ghx_uput_segment": (c_i32, [c_vp, c_i32, P(UPutSegmentInfo)]),
    "ghx_epochs_create": (c_i32, [ctypes.c_char_p, c_i32, c_i32, c_i32, ctypes.c_double, P(c_vp)]),
    "ghx_epochs_unlink": (c_i32, [ctypes.c_char_p]),
    "ghx_epochs_peers": (c_i32, [c_vp, P(c_i32), c_i32, P(c_i32), c_i32]),
    "ghx_epochs_enqueue": (c_i32, [c_vp, c_i32, c_vp]),
    "ghx_epochs_status": (c_i32, [c_vp, P(c_i32), P(ctypes.c_uint64)]),
    "ghx_epochs_info": (c_i32, [c_vp, P(c_i32), P(c_i32)]),
    "ghx_epochs_counter": (c_i32, [c_vp, P(c_vp)]),
    "ghx_exchange_set_parity": (c_i32, [c_vp, c_i32, c_vp, ctypes.c_uint32, P(ctypes.c_int64), c_i32]),
    "ghx_epochs_destroy": (c_i32, [c_vp]),
    "ghx_copier_create": (c_i32, [ctypes.c_uint64, ctypes.c_double, P(c_vp)]),
    "ghx_copier_info": (c_i32, [c_vp, P(c_i32), P(c_i32), P(ctypes.c_float), P(ctypes.c_float),
                                P(ctypes.c_float)]),
    "ghx_copier_submit": (c_i32, [c_vp, c_vp, c_vp, ctypes.c_uint64, c_i32, ctypes.c_int64,
                                  P(ctypes.c_uint64)]),
    "ghx_copier_wait": (c_i32, [c_vp, ctypes.c_uint64]),
    "ghx_copier_acquire": (c_i32, [c_vp, c_vp]),
    "ghx_copier_destroy": (c_i32, [c_vp]),
}
# the six adjoint families' create, reverse pack and accumulate take the same arguments
for _prefix in ("ghx_uexchange_adjoint", "ghx_uexchange_adjoint_self", "ghx_sexchange_adjoint",
                "ghx_sexchange_adjoint_self", "ghx_cs_exchange_adjoint", "ghx_cs_exchange_adjoint_self"):
    _SIGS[_prefix + "_create"] = (c_i32, [c_vp, P(c_i32), c_i32])
    _SIGS[_prefix + "_pack"] = (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_vp])
    _SIGS[_prefix + "_accumulate"] = (c_i32, [c_vp, P(c_vp), c_i32, P(c_vp), c_i32, c_i32, c_vp])
EXPORTED = tuple(_SIGS)

_lib = None


class GhxError(RuntimeError):
    """A failed ghx_* call (the reference raises std::runtime_error)."""


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"ghex_amd native library missing: {LIB_PATH}. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                "There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().ghx_last_error().decode()
        raise GhxError(f"{what} failed ({rc}): {msg}")


def call(name, *args):
    check(getattr(lib(), name)(*args), name)


def ptr_array(ptrs):
    arr = (c_vp * max(1, len(ptrs)))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


def i32_array(vals):
    return (c_i32 * max(1, len(vals)))(*vals)


def i64_array(vals):
    return (c_i64 * max(1, len(vals)))(*vals)


def i64_ptr(a):
    """ctypes int64* into a C-contiguous numpy int64 array (kept alive by the caller)."""
    return a.ctypes.data_as(ctypes.POINTER(c_i64))
