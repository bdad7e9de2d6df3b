"""ghex_amd.structured.cubed_sphere — the cubed-sphere grid of the reference
(include/ghex/structured/cubed_sphere/{transform,domain_descriptor,halo_generator,
field_descriptor}.hpp) on the MI355X-native path.

Six tiles of edge_size x edge_size cells over `levels` levels, oriented as drawn in
cubed_sphere/transform.hpp:21-38. Domains are rectangles of one tile; a halo that crosses a cube
edge is packed by the neighbour in its own coordinates and rotated (vector components also
sign-flipped) by the receiver's unpack, which libghx runs as a second launch after the ordinary
unpack (k_unpack_x). Fields are used with the ordinary CommunicationObject, or with this module's
make_bulk_communication_object (zero-copy rotating puts between node-local ranks); the plain
bulk object and the direct and pipelined exchanges refuse them."""
from __future__ import annotations

import ctypes
from typing import Sequence

from .. import _ghx
from ..communication_object import CommunicationObject
from ..pattern import PatternContainer
from .regular import _layout_order


def make_communication_object(context, fuse_rotated: bool = False, adjoint_rotated: bool = False,
                              fuse_adjoint_rotated: bool = False, **options) -> CommunicationObject:
    """The plain communication object. fuse_rotated=True (opt-in): an exchange whose every
    message stays on this rank (a whole cube on one rank) runs as ONE launch that packs and
    rotates (ghx_cs_exchange_self); any other exchange takes the usual three launches.
    adjoint_rotated=True (opt-in): adjoint_exchange and its siblings take cubed-sphere fields
    (ghx_cs_exchange_adjoint_*: a reverse pack that rotates and negates, then the accumulate).
    fuse_adjoint_rotated=True (opt-in, with adjoint_rotated): the adjoint adds the halo cells of
    self messages straight into their owner cells, through the edge's transform, in the accumulate
    launch (ghx_cs_exchange_adjoint_self_*, k_accum_get_x); their buffers are not touched. A whole
    cube on one rank then runs its adjoint as ONE launch."""
    return CommunicationObject(context, fuse_rotated=fuse_rotated, adjoint_rotated=adjoint_rotated,
                               fuse_adjoint_rotated=fuse_adjoint_rotated, **options)


def make_bulk_communication_object(context, epochs: str = "device", timeout: float = 30.0,
                                   remote_options=None):
    """The zero-copy (bulk) exchange for cubed-sphere fields: every rank puts its send regions
    straight into the node-local receivers' halos, rotated and sign-flipped on the way
    (ghx_cs_put_create, one k_put_cs launch per group of <= 64 messages) — no send or receive
    buffers. Takes cubed-sphere fields of 1-, 2-, 4-, 8- or 16-byte elements only; epochs,
    timeout and remote_options as bulk_communication_object.make_bulk_communication_object (the
    halos of ranks on other hosts travel through a buffered cubed-sphere exchange)."""
    from ..bulk_communication_object import BulkCommunicationObject
    return BulkCommunicationObject(context, epochs=epochs, timeout=timeout,
                                   remote_options=remote_options, cubed_sphere=True)


class Cube:
    """cubed_sphere::cube {edge_size, levels} (domain_descriptor.hpp:22-30)."""

    def __init__(self, edge_size: int, levels: int):
        self.edge_size, self.levels = int(edge_size), int(levels)
        if self.edge_size < 1 or self.levels < 1:
            raise ValueError("edge_size and levels must be >= 1")

    def __repr__(self):
        return f"Cube({self.edge_size}, {self.levels})"


class DomainDescriptor:
    """cubed_sphere::domain_descriptor(cube, tile, x_first, x_last, y_first, y_last)
    (domain_descriptor.hpp:69-111). first()/last() are the 3-D (x, y, z) corners on the tile.
    The id is computed, not chosen: (tile * c + y_first) * c + x_first, whose integer order is
    the reference's (tile, (x_first, y_first)) order (:33-61)."""

    ndim = 3

    def __init__(self, cube: Cube, tile: int, x_first: int, x_last: int, y_first: int,
                 y_last: int):
        self.cube = cube
        self.tile = int(tile)
        self.x_first, self.x_last = int(x_first), int(x_last)
        self.y_first, self.y_last = int(y_first), int(y_last)
        c = cube.edge_size
        if not 0 <= self.tile <= 5:
            raise ValueError("tile must be in 0..5")
        if not (0 <= self.x_first <= self.x_last < c and 0 <= self.y_first <= self.y_last < c):
            raise ValueError("the domain must lie inside its tile")

    def domain_id(self) -> int:
        c = self.cube.edge_size
        return (self.tile * c + self.y_first) * c + self.x_first

    def edge_size(self) -> int:
        return self.cube.edge_size

    def first(self):
        return (self.x_first, self.y_first, 0)

    def last(self):
        return (self.x_last, self.y_last, self.cube.levels - 1)

    def _c(self, rank=0):
        d = _ghx.CsDomain()
        d.rank, d.tile = rank, self.tile
        d.x_first, d.x_last, d.y_first, d.y_last = (self.x_first, self.x_last, self.y_first,
                                                    self.y_last)
        return d

    def __repr__(self):
        return (f"DomainDescriptor({self.cube}, {self.tile}, {self.x_first}, {self.x_last}, "
                f"{self.y_first}, {self.y_last})")


class HaloGenerator:
    """cubed_sphere::halo_generator (halo_generator.hpp:56-198): one width, or four applied as
    the reference's code applies them: -x, +x, -y, +y."""

    def __init__(self, halo):
        if isinstance(halo, int):
            halo = (halo,) * 4
        self.halos = tuple(int(h) for h in halo)
        if len(self.halos) != 4 or min(self.halos) < 0:
            raise ValueError("need one halo width or four (-x, +x, -y, +y), all >= 0")

    def __call__(self, domain: DomainDescriptor):
        """The receive boxes of `domain` in generation order:
        [(local_first, local_last, global_first, global_last, tile)], 3-D (x, y, z); the global
        box is in the coordinates of `tile` (the domain's own or an edge neighbour's)."""
        cube = domain.cube
        n = ctypes.c_int32()
        d = domain._c()
        args = (cube.edge_size, cube.levels, ctypes.byref(d), _ghx.i32_array(self.halos))
        _ghx.call("ghx_cs_halo_boxes", *args, None, None, None, 0, ctypes.byref(n))
        loc = (_ghx.Box * max(1, n.value))()
        glo = (_ghx.Box * max(1, n.value))()
        til = (ctypes.c_int32 * max(1, n.value))()
        _ghx.call("ghx_cs_halo_boxes", *args, loc, glo, til, n.value, ctypes.byref(n))
        return [(tuple(loc[i].first[:3]), tuple(loc[i].last[:3]), tuple(glo[i].first[:3]),
                 tuple(glo[i].last[:3]), int(til[i])) for i in range(n.value)]


def make_pattern(context, halo_gen: HaloGenerator, domain_range: Sequence[DomainDescriptor]):
    """make_pattern<structured::grid>(context, halo_gen, domains) with the cubed-sphere halo
    generator (include/ghex/structured/pattern.hpp:214-571, cubed_sphere/halo_generator.hpp
    :227-283). All ranks' domains are all-gathered once; libghx derives this rank's maps."""
    domain_range = list(domain_range)
    if not domain_range:
        raise ValueError("need at least one domain")
    cube = domain_range[0].cube
    mine = [(d.cube.edge_size, d.cube.levels, d.tile, d.x_first, d.x_last, d.y_first, d.y_last)
            for d in domain_range]
    gathered = context.all_gather_object(mine)
    doms = []
    for r, lst in enumerate(gathered):
        for (c, lev, t, xf, xl, yf, yl) in lst:
            if (c, lev) != (cube.edge_size, cube.levels):
                raise ValueError("all domains must belong to the same cube")
            d = _ghx.CsDomain()
            d.rank, d.tile, d.x_first, d.x_last, d.y_first, d.y_last = r, t, xf, xl, yf, yl
            doms.append(d)
    darr = (_ghx.CsDomain * len(doms))(*doms)
    h = ctypes.c_void_p()
    _ghx.call("ghx_cs_pattern_create", cube.edge_size, cube.levels, darr, len(doms),
              _ghx.i32_array(halo_gen.halos), context.rank(), ctypes.byref(h))
    return PatternContainer(h.value, context, domain_range, "structured", 3)


def _value_kind(tensor) -> int:
    """How a vector component is negated: 1 IEEE float (sign bit), 2 signed integer, 0 neither."""
    if tensor.is_floating_point():
        return 1
    name = str(tensor.dtype)
    return 2 if name in ("torch.int32", "torch.int64") else 0


class FieldDescriptor:
    """cubed_sphere::field_descriptor over a device tensor (cubed_sphere/field_descriptor.hpp
    :26-225): a tensor indexed (x, y, z) or (x, y, z, component) in any memory layout.
    is_vector_field: components 0 and 1 are the x and y components of a vector, negated where
    the neighbour tile's axes point the other way (:97-104)."""

    kind = 0

    def __init__(self, domain: DomainDescriptor, field, offsets, extents, num_components=1,
                 is_vector_field=False):
        from ..util import as_device_tensor
        field = as_device_tensor(field)
        if field.device.type != "cuda":
            raise TypeError("ghex_amd fields live in device memory (torch device 'cuda')")
        nd = field.dim()
        if nd not in (3, 4):
            raise ValueError(f"a cubed-sphere field has 3 dims (x, y, z) or 4 (with components), "
                             f"got {nd}")
        self.domain = domain
        self.tensor = field
        self.has_components = nd == 4
        self.num_components = int(field.shape[-1]) if self.has_components else 1
        if int(num_components) != self.num_components:
            raise ValueError("num_components does not match the field's last dimension")
        self.is_vector_field = bool(is_vector_field)
        itemsize = field.element_size()
        strides = tuple(int(s) * itemsize for s in field.stride())
        self.layout = _layout_order(strides)
        offs = list(offsets) + ([0] if self.has_components else [])
        exts = list(extents) + ([self.num_components] if self.has_components else [])
        if len(offs) != nd or len(exts) != nd:
            raise ValueError("offsets/extents must have one entry per spatial dimension")
        for d in range(nd):
            if int(field.shape[d]) < exts[d]:
                raise ValueError("field smaller than its declared extents")
        fd = _ghx.FieldDesc()
        fd.dim, fd.elem_size = nd, itemsize
        for d in range(nd):
            fd.layout[d] = self.layout[d]
            fd.byte_strides[d] = strides[d]
            fd.offsets[d] = int(offs[d])
            fd.extents[d] = int(exts[d])
        fd.num_components = self.num_components
        fd.has_components = 1 if self.has_components else 0
        self.desc = fd
        self.align = itemsize
        self.offsets = tuple(offs)
        self.extents = tuple(exts)
        cs = _ghx.CsItem()
        cs.tile, cs.first_x, cs.first_y = domain.tile, domain.x_first, domain.y_first
        cs.edge_size = domain.cube.edge_size
        cs.is_vector = 1 if self.is_vector_field else 0
        cs.value_kind = _value_kind(field)
        if self.is_vector_field and not (cs.value_kind in (1, 2) and itemsize in (4, 8)):
            raise ValueError("a cubed-sphere vector field must hold 4- or 8-byte floats or signed "
                             "integers")
        self.cs_item = cs

    def domain_id(self) -> int:
        return self.domain.domain_id()

    def edge_size(self) -> int:
        return self.domain.cube.edge_size

    def dtype_code(self) -> int:
        """The element type code of the adjoint exchange (GHX_DT_*), as
        regular.FieldDescriptor.dtype_code. TypeError for a dtype it does not sum."""
        import torch
        codes = {torch.float32: _ghx.DT_F32, torch.float64: _ghx.DT_F64,
                 torch.int32: _ghx.DT_I32, torch.int64: _ghx.DT_I64}
        code = codes.get(self.tensor.dtype)
        if code is None:
            raise TypeError(f"adjoint exchange: dtype {self.tensor.dtype} is not supported "
                            "(float32, float64, int32, int64)")
        return code

    def data_ptr(self) -> int:
        return self.tensor.data_ptr()

    @property
    def device(self):
        return self.tensor.device

    @staticmethod
    def _boxes(spaces, lo, hi):
        arr = (_ghx.Box * max(1, len(spaces)))()
        for i, sp in enumerate(spaces):
            for d in range(3):
                arr[i].first[d], arr[i].last[d] = sp[lo][d], sp[hi][d]
        return arr

    def pack(self, buffer, spaces, stream=None):
        """field.pack(buffer, index_container, stream) (field_descriptor.hpp:130-140): the
        ordinary pack of the spaces' local boxes."""
        import torch
        s = (stream or torch.cuda.current_stream()).cuda_stream
        bp = buffer.data_ptr() if hasattr(buffer, "data_ptr") else int(buffer)
        _ghx.call("ghx_structured_pack", ctypes.byref(self.desc), self.data_ptr(), bp,
                  self._boxes(spaces, 0, 1), len(spaces), s)

    def unpack(self, buffer, spaces, stream=None):
        """field.unpack(buffer, index_container, stream) (field_descriptor.hpp:142-167).
        spaces: [(local_first, local_last, global_first, global_last, tile)]."""
        import torch
        s = (stream or torch.cuda.current_stream()).cuda_stream
        bp = buffer.data_ptr() if hasattr(buffer, "data_ptr") else int(buffer)
        tiles = _ghx.i32_array([int(sp[4]) for sp in spaces])
        _ghx.call("ghx_cs_unpack", ctypes.byref(self.desc), ctypes.byref(self.cs_item),
                  self.data_ptr(), bp, self._boxes(spaces, 0, 1), self._boxes(spaces, 2, 3),
                  tiles, len(spaces), s)

    def pack_rotated(self, buffer, spaces, stream=None):
        """The transpose of unpack (ghx_cs_pack_rotated): the field's cells of the spaces' local
        boxes go to the buffer positions unpack reads them from, negated where unpack negates.
        The field is read, the buffer written; spaces as unpack takes them."""
        import torch
        s = (stream or torch.cuda.current_stream()).cuda_stream
        bp = buffer.data_ptr() if hasattr(buffer, "data_ptr") else int(buffer)
        tiles = _ghx.i32_array([int(sp[4]) for sp in spaces])
        _ghx.call("ghx_cs_pack_rotated", ctypes.byref(self.desc), ctypes.byref(self.cs_item),
                  self.data_ptr(), bp, self._boxes(spaces, 0, 1), self._boxes(spaces, 2, 3),
                  tiles, len(spaces), s)


def make_field_descriptor(domain_desc: DomainDescriptor, field, offsets, extents,
                          num_components=1, is_vector_field=False, *, arch=None):
    from ..util import check_arch
    check_arch(arch)
    return FieldDescriptor(domain_desc, field, offsets, extents, num_components, is_vector_field)
