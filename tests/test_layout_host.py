"""CPU: the arena's offset rule and the rasterizer call's buffer layout (``ops._layout_a`` / ``_layout_b`` / ``_layout_bwd``).
The calls carve FROM a layout and reserve the demand OF it; what can go wrong without a GPU is the rule itself, the
agreement of the two, and the order of the arrays (where an array lies in the slot is measured: arena.py)."""
import ctypes as C
import itertools
import os
import zlib

import pytest
import torch

from collab_splats_amd import _lib, arena, ops

PKG = os.path.dirname(ops.__file__)


def test_offset_rule_on_hand_computed_sequences():
    """``arena.place`` is what ``Slot.take`` and the shadow count of ``Carver.take`` did: round the offset up to 256 bytes,
    then add the bytes -- also for an empty take (it still moves the offset to the boundary) and around ``BIG``."""
    BIG = arena.BIG
    assert (arena.ALIGN_SMALL, arena.ALIGN_BIG, BIG) == (256, 256, 1 << 20)
    assert arena.place(0, 100) == (0, 100)
    assert arena.place(100, 0) == (256, 256)                              # a zero-size take
    assert arena.place(256, BIG) == (256, 256 + BIG)                      # exactly BIG bytes
    assert arena.place(256 + BIG, BIG - 1) == (1048832, 2097407)          # BIG - 1
    assert arena.place(2097407, 4) == (2097408, 2097412)
    assert arena.place(511, 1) == (512, 513) and arena.place(512, 1) == (512, 513)
    assert arena.demand([100, 0, BIG, BIG - 1, 4]) == 2097412
    assert arena.demand([]) == 0 and arena.demand([0]) == 0 and arena.demand([1, 1, 1]) == 513
    # ... and a slot counts with it, past its own end too (the demand of the whole call)
    if arena._use_count is not None:
        s = arena.Slot(torch.device("cpu"), 1024)
        assert s.take(25, torch.float32).numel() == 25 and (s.off, s.demand) == (100, 100)
        assert s.take(0, torch.int32).numel() == 0 and s.off == 256 and s.served_all()
        assert s.take(300, torch.float32) is None and (s.off, s.demand) == (1456, 1456) and not s.served_all()


class _Recorder:
    """A carver that hands out CPU memory and counts with the offset rule, take by take."""
    dev = torch.device("cpu")

    def __init__(self):
        self.off = 0

    def take(self, count, dtype):
        self.off = arena.place(self.off, count * arena._ESIZE[dtype])[1]
        return torch.empty(count, dtype=dtype)


def _cases():
    for cams, grad, absgrad, (nxq, lazy), indexed, keyed, aux in itertools.product(
            (1, 2), (False, True), (False, True), ((0, False), (0, True), (3, False), (3, True), (4, False), (4, True)),
            (False, True), (False, True), (False, True)):
        if (absgrad or aux) and not grad:
            continue
        yield cams, grad, absgrad, nxq, lazy, indexed, keyed, aux


def test_layout_demand_is_what_its_takes_add_up_to():
    """For every combination of the switches the layout depends on (N = 3000, one and two cameras, 96 x 64): the demand the
    layout reports -- the figure ``reserve`` gets -- equals what carving it array by array asks of the arena, every array
    has its element count, and the range the projection kernel clears is contiguous."""
    n = 0
    for cams, grad, absgrad, nxq, lazy, indexed, keyed, aux in _cases():
        P = _lib.make_params(3000, cams, 96, 64)
        cd = 4 if nxq == 0 else 4 + 4 * nxq
        front = keyed and indexed
        takes = ops._layout_a(P, 24, 12, grad, aux, absgrad, nxq, lazy, indexed) + ops._layout_b(P, keyed, front, cd, 8192)
        rec = _Recorder()
        got = ops._carve_all(rec, takes)
        assert rec.off == ops._demand(takes), (cams, grad, absgrad, nxq, lazy, indexed, keyed, aux)
        assert [(k, v.numel(), v.dtype) for k, v in got.items()] == [(t.name, t.count, t.dtype) for t in takes]
        assert ("v_grec_zero" in got) == grad and ("v_abs_zero" in got) == absgrad and ("unit_work" in got) == keyed
        assert ("featx" in got) == (nxq > 0 and not lazy) and ("v_featx_zero" in got) == (nxq > 0 and grad)
        assert got["depth_sorted"].numel() == (3000 * cams if indexed else 0) and got["front_n"].numel() == (24 * cams if front else 0)
        p0 = got["cell_count"].data_ptr()
        assert [got[k].data_ptr() - p0 for k in ("cell_cursor", "counters", "tile_count")] == [4 * 64, 8 * 64, 12 * 64]
        n += 1
    assert n > 100


def test_layout_order_is_pinned():
    """The order and the grouping of the arrays, written out: a reordering moves arrays inside the slot (measured placement)."""
    f, i = torch.float32, torch.int32
    P = _lib.make_params(3000, 1, 96, 64)
    a = ops._layout_a(P, 24, 12, True, True, False, 0, False, False)
    b = ops._layout_b(P, True, False, 4, 8192)
    assert [(t.name, t.count) for t in a] == [
        ("means2d", 6000), ("depths", 3000), ("comps", 3000), ("sh_aux", 36000), ("grec", 48000), ("v_grec_zero", 48000),
        ("radii", 6000), ("tiles_per_gauss", 3000), ("rect2", 6000), ("cellhist", 288), ("cell_count", 24), ("cell_cursor", 24),
        ("counters", 4), ("tile_count", 25), ("cell_offs", 25), ("order", 3000), ("rect_sorted", 6000), ("touched", 750),
        ("depth_sorted", 0)]
    assert [t.carve for t in a] == [0, 0, 0, 0, -1, -1] + [1] * 13
    assert [t.dtype for t in a] == [f] * 6 + [i] * 13
    assert [(t.name, t.count) for t in b] == [
        ("render", 24576), ("alpha", 6144), ("exp_depth", 6144), ("med_depth", 6144), ("normal", 18432), ("unit_work", 48),
        ("unit_perm", 0), ("last_ids", 6144), ("median_ids", 6144), ("offsets", 26), ("reach", 48), ("front_n", 0), ("tile_flag", 0),
        ("payload", 8192), ("flatten_ids", 8192), ("scratch", 16384)]
    assert [t.carve for t in b] == [0] * 5 + [1, 1] + [2] * 6 + [-1] * 3
    assert [t.dtype for t in b] == [f] * 5 + [i] * 11
    # the pieces as the arena sees them: 64-element rounding inside a carve, the exact count of a take of its own
    assert [(n, len(ts)) for _, n, ts in ops._pieces(a + b)] == [
        (6016 + 3008 + 3008 + 36032, 4), (48000, 1), (48000, 1),
        (6016 + 3008 + 6016 + 320 + 64 + 64 + 64 + 64 + 64 + 3008 + 6016 + 768 + 0, 13),
        (24576 + 3 * 6144 + 18432, 5), (64, 2), (6144 + 6144 + 64 + 64, 6), (8192, 1), (8192, 1), (16384, 1)]
    # two cameras, absgrad, the features model's call with its own featx rows, front-only ordering, no SH Jacobian
    P = _lib.make_params(3000, 2, 96, 64)
    a = ops._layout_a(P, 24, 12, True, False, True, 3, False, True)
    b = ops._layout_b(P, True, True, 16, 8192)
    assert [(t.name, t.count) for t in a] == [
        ("means2d", 12000), ("depths", 6000), ("comps", 6000), ("sh_aux", 0), ("grec", 96000), ("v_grec_zero", 96000),
        ("v_abs_zero", 12000), ("featx", 72000), ("v_featx_zero", 72000), ("radii", 12000), ("tiles_per_gauss", 6000),
        ("rect2", 12000), ("cellhist", 288), ("cell_count", 24), ("cell_cursor", 24), ("counters", 4), ("tile_count", 49),
        ("cell_offs", 25), ("order", 6000), ("rect_sorted", 12000), ("touched", 1500), ("depth_sorted", 6000)]
    assert [(t.name, t.count) for t in b] == [
        ("render", 196608), ("alpha", 12288), ("exp_depth", 12288), ("med_depth", 12288), ("normal", 36864), ("unit_work", 96),
        ("unit_perm", 0), ("last_ids", 12288), ("median_ids", 12288), ("offsets", 50), ("reach", 96), ("front_n", 48),
        ("tile_flag", 48), ("payload", 8192), ("flatten_ids", 8192), ("scratch", 16384)]
    # without a view-keyed order table the schedule's arrays are not the slot's, and nothing is measured per unit
    b = ops._layout_b(P, False, False, 16, 8192)
    assert [t.name for t in b][5:8] == ["last_ids", "median_ids", "offsets"] and b[8] == ops.Take("reach", i, 0, 2)


def test_backward_layout_follows_what_the_call_allocates():
    counts = [9000, 135000, None, 9000, 12000, 9000, 3000]
    lay = ops._layout_bwd(3000, 0, counts, 9000, False, False, True)
    assert [(t.name, t.count) for t in lay] == [
        ("v_colors", 9000), ("v_colors_rest", 135000), ("v_means_dir", 9000), ("v_means", 9000), ("v_quats", 12000),
        ("v_scales", 9000), ("v_opac", 3000), ("v_m2d", 6000)]
    assert all(t.carve == -1 and t.dtype == torch.float32 for t in lay)
    assert ops._demand(lay) == arena.demand([4 * t.count for t in lay])
    # rows the forward did not clear, a features tensor, no SH, a sink that owns the geometry gradients, nobody holds means2d
    lay = ops._layout_bwd(3000, 3, [0, None, 39000, None, None, None, None], None, True, True, False)
    assert [(t.name, t.count) for t in lay] == [("v_grec", 48000), ("v_colors", 0), ("v_features", 39000), ("v_featx", 36000)]
    rec = _Recorder()
    assert list(ops._carve_all(rec, lay)) == [t.name for t in lay] and rec.off == ops._demand(lay)


@pytest.mark.parametrize("simple,sparse,have", list(itertools.product((False, True), repeat=3)))
def test_packed_rows_are_the_mean_gradient_except_after_flagged_rows(simple, sparse, have):
    """After a one-call flagged-rows backward columns 0:2 of the packed rows hold sums, not the screen-space gradient:
    ``meta["means2d"].grad`` may be read from them in every other case only."""
    assert ops._rows_hold_mean_gradient(simple, sparse, have) == (not (simple and sparse and not have))


def test_remedy_texts_name_the_module_switch():
    for name in ("ops.py", "graphs.py"):
        with open(os.path.join(PKG, name)) as fh:
            text = fh.read()
        assert "MISPLAT_FUSED_NODE" not in text, name
    with open(os.path.join(PKG, "ops.py")) as fh:
        assert fh.read().count("collab_splats_amd.ops.FUSED_NODE = False") == 2
    with open(os.path.join(PKG, "graphs.py")) as fh:
        assert "FUSED_NODE left True" in fh.read()


def test_argument_blocks_keep_their_size_and_field_offsets():
    """The C entries receive the same blocks as before the layout moved into one place: sizes and every field offset."""
    def image(cls):
        return zlib.crc32(";".join("%s:%d:%d" % (f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size)
                                   for f in cls._fields_).encode())
    got = {c.__name__: (C.sizeof(c), len(c._fields_), image(c)) for c in (_lib.Params, _lib.RasterArgs, _lib.RasterBwdArgs)}
    assert got == {"Params": PARAMS, "RasterArgs": RASTER_ARGS, "RasterBwdArgs": RASTER_BWD_ARGS}, got


# (bytes, fields, CRC-32 of "name:offset:size;..." over the fields in order)
PARAMS = (168, 34, 2037685776)
RASTER_ARGS = (488, 68, 3459940446)
RASTER_BWD_ARGS = (408, 58, 1260733510)
