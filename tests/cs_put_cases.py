"""Shared set-up of the cubed-sphere put tests: emulated ranks of one process that plan their puts
as the bulk object does (field_records -> put_messages -> put_chunks -> put_entries + cs_put_args
-> ghx_cs_put_create), over fields that are plain descriptors and pointers. Works without a
device (pointers 0: the plans can be described, not executed)."""
from __future__ import annotations

import ctypes

from tests import cs_cases
from tests.gpu_util import FakeContext

X_FAST, Y_FAST, Z_FAST, K_FAST = (3, 2, 1, 0), (2, 3, 1, 0), (1, 2, 3, 0), (0, 1, 2, 3)


def field_shape(cfg, dom, nc, pad=1):
    """DomainField's shape and offsets: `pad` untouched cells beyond the widest halo in x and y."""
    h = max(cfg["halos"]) + pad
    return ((dom["x"][1] - dom["x"][0] + 1 + 2 * h, dom["y"][1] - dom["y"][0] + 1 + 2 * h,
             cfg["levels"], nc), (h, h, 0, 0))


def field_desc(shape, offsets, layout, elem, strides=None):
    from ghex_amd import _ghx
    fd = _ghx.FieldDesc()
    fd.dim, fd.elem_size, fd.num_components, fd.has_components = 4, elem, shape[3], 1
    strides = strides or cs_cases.dense_strides(shape, layout, elem)
    for d in range(4):
        fd.layout[d], fd.byte_strides[d] = layout[d], strides[d]
        fd.offsets[d], fd.extents[d] = offsets[d], shape[d]
    return fd


def cs_item(cfg, dom, vector, kind):
    from ghex_amd import _ghx
    cs = _ghx.CsItem()
    cs.tile, cs.first_x, cs.first_y = dom["tile"], dom["x"][0], dom["y"][0]
    cs.edge_size, cs.is_vector, cs.value_kind = cfg["edge_size"], 1 if vector else 0, kind
    return cs


class Field:
    """What the bulk planning reads of a field: descriptor, cubed-sphere item, domain id, pointer."""

    kind = 0

    def __init__(self, desc, cs, did, ptr=0):
        self.desc, self.cs_item, self._did, self._ptr = desc, cs, did, ptr
        self.align = desc.elem_size

    def domain_id(self):
        return self._did

    def data_ptr(self):
        return self._ptr


def value_kind(dtype, vector):
    return {"f": 1, "i": 2}.get(cs_cases.elem_kind(dtype), 0) if vector else 0


def emulated_ranks(cfg, rank_of):
    """rank_of(i, domain) -> rank. Per rank: (domain indices, DomainDescriptors, pattern)."""
    from ghex_amd.structured import cubed_sphere as CS
    cube = CS.Cube(cfg["edge_size"], cfg["levels"])
    ranks = [rank_of(i, d) for i, d in enumerate(cfg["domains"])]
    world = max(ranks) + 1
    mine = [[i for i, r in enumerate(ranks) if r == q] for q in range(world)]
    table = [[(cube.edge_size, cube.levels, cfg["domains"][i]["tile"], *cfg["domains"][i]["x"],
               *cfg["domains"][i]["y"]) for i in mine[q]] for q in range(world)]
    out = []
    for q in range(world):
        dds = [CS.DomainDescriptor(cube, cfg["domains"][i]["tile"], *cfg["domains"][i]["x"],
                                   *cfg["domains"][i]["y"]) for i in mine[q]]
        pc = CS.make_pattern(FakeContext(q, world, table), CS.HaloGenerator(cfg["halos"]), dds)
        out.append((mine[q], dds, pc))
    return out


class Puts:
    """Every emulated rank's put plans over bis_all[r] (buffer infos of Field-like fields, same
    order on every rank): plans[r] = [(handle, source pointers, n, target pointers, n)].
    mutate(src entries, dst entries) may change a request before it is planned. dst_ptrs[r][i]:
    where rank r's field i is written, if not where it is read (the fields' own pointers)."""

    def __init__(self, bis_all, mutate=None, dst_ptrs=None):
        from ghex_amd import _ghx
        from ghex_amd import bulk_communication_object as B
        self.ghx = _ghx
        groups = [B.field_groups(bis) for bis in bis_all]
        allr = [{"host": "h", "fields": B.field_records(bis, g, export=False)}
                for bis, g in zip(bis_all, groups)]
        local = list(range(len(bis_all)))
        self.plans, self._keep = [], []
        for r, bis in enumerate(bis_all):
            mine = []
            for chunk, srcs, dsts in B.put_chunks(B.put_messages(bis, groups[r], allr, local)):
                src, dst, keep = B.put_entries(chunk, srcs, dsts, [bi.field.desc for bi in bis],
                                               allr)
                items, gptr, tptr, more = B.cs_put_args(chunk, allr)
                self._keep += [keep, more]
                h = ctypes.c_void_p()
                n = len(chunk)
                if mutate is not None:
                    mutate(src, dst)
                _ghx.call("ghx_cs_put_create", src, n, dst, n, items, gptr, tptr, ctypes.byref(h))
                sp = _ghx.ptr_array([bis[k].field.data_ptr() for k in srcs])
                dp = _ghx.ptr_array([dst_ptrs[tr][ti] if dst_ptrs else
                                     bis_all[tr][ti].field.data_ptr() for tr, ti in dsts])
                mine.append((h, sp, len(srcs), dp, len(dsts)))
            self.plans.append(mine)

    def handles(self):
        return [p[0] for mine in self.plans for p in mine]

    def info(self):
        """Summed over all plans: message bytes, tiles, pair tiles, put tile records, put tiles."""
        tot = dict(bytes=0, tiles=0, pair_tiles=0, records=0, x_tiles=0)
        for h in self.handles():
            b, t = ctypes.c_uint64(), ctypes.c_int32()
            p, r, x = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
            self.ghx.call("ghx_put_info", h, ctypes.byref(b), ctypes.byref(t))
            self.ghx.call("ghx_cs_put_info", h, ctypes.byref(p), ctypes.byref(r), ctypes.byref(x))
            assert t.value == p.value + x.value
            for k, v in zip(tot, (b, t, p, r, x)):
                tot[k] += v.value
        return tot

    def execute(self, stream):
        for mine in self.plans:
            for h, sp, ns, dp, nd in mine:
                self.ghx.call("ghx_put_execute", h, sp, ns, dp, nd, stream)

    def close(self):
        for h in self.handles():
            self.ghx.lib().ghx_put_destroy(h)
        self.plans = []


def descriptor_fields(cfg, rank_of, specs):
    """Device-less: bis_all for `specs` = [(layout or function of the domain index, elem, nc,
    vector, kind)] fields per domain, spec-major on every rank."""
    bis_all = []
    for mine, dds, pc in emulated_ranks(cfg, rank_of):
        bis = []
        for layout, elem, nc, vector, kind in specs:
            for i, dd in zip(mine, dds):
                dom = cfg["domains"][i]
                shape, offs = field_shape(cfg, dom, nc)
                lay = layout(i) if callable(layout) else layout
                bis.append(pc(Field(field_desc(shape, offs, lay, elem),
                                    cs_item(cfg, dom, vector, kind), dd.domain_id())))
        bis_all.append(bis)
    return bis_all
