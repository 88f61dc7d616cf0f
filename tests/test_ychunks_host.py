"""``stack_detect._zy_chunks``: the out-of-core planner that cuts a layer of blocks too large for the device into runs of
whole block rows (no GPU); ``_host_chunks``, ``_share_box`` and ``_chunk_cells``, the one plan by which any host image goes
up; and ``volume._plane_pitch``, which tells the staged upload how a box of a host image lies."""
import numpy as np
import pytest


def _grid(shape, segment_size):
    from magellanmapper_amd import config, roi_prof, stack_detect as sd
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    blocks = sd.setup_blocks(roi_prof.ROIProfile(segment_size=segment_size, denoise_size=None), shape)
    return blocks, sd.StackDetector._grid_coords(blocks.sub_roi_slices.shape)


def _limits(shape, origins, shapes, row_bytes):
    """Byte limits from "everything fits" down to "one block row does not fit", from the grid's own extents: T planes in
    the thickest layer, R rows in the tallest block row, R2 in the tallest pair of neighbouring block rows."""
    t = max(s[0] for s in shapes)
    y_ext = sorted({(o[1], o[1] + s[1]) for o, s in zip(origins, shapes)})
    r = max(b - a for a, b in y_ext)
    r2 = max([d[1] - c[0] for c, d in zip(y_ext, y_ext[1:])] + [r])
    whole = shape[0] * shape[1] * row_bytes
    return {"all": 2 * whole, "two_layers": 2 * 2 * t * shape[1] * row_bytes, "layer": 2 * t * shape[1] * row_bytes,
            "layer_less_a_row": 2 * t * (shape[1] - 1) * row_bytes, "two_rows": 2 * t * r2 * row_bytes,
            "row": 2 * t * r * row_bytes, "row_less_one": 2 * t * (r - 1) * row_bytes, "tiny": 2 * 10 * row_bytes}


# (the first grid is that of test_z_chunks_are_whole_block_layers_within_the_byte_limit: two block rows per layer; the
#  second has six, so that runs of several block rows are merged and then end)
@pytest.mark.parametrize("shape,segment_size", [((230, 90, 100), 50), ((90, 230, 80), 40)])
def test_zy_chunks_cut_an_oversized_layer_into_runs_of_whole_block_rows(shape, segment_size):
    """Contiguous k-ranges that cover the share once; every block inside its chunk's box; a chunk with cut rows holds whole
    block rows of exactly one layer; a box takes at most ``limit // 2`` bytes unless it is a single block row; with every
    layer fitting the result is ``_z_chunks``' with full rows."""
    from magellanmapper_amd import stack_detect as sd
    blocks, coords = _grid(shape, segment_size)
    n_rows, row_bytes = shape[1], shape[2] * 2
    plane = n_rows * row_bytes
    seen_cut = seen_merged = seen_oversized = 0
    for mine in (list(range(len(coords))), list(range(5, len(coords) - 3))):
        origins, shapes = sd.StackDetector._block_extents(blocks.sub_roi_slices, shape, mine)
        limits = _limits(shape, origins, shapes, row_bytes)
        for name, limit in limits.items():
            chunks = sd._zy_chunks(coords, mine, origins, shapes, plane, row_bytes, limit)
            z_only = sd._z_chunks(coords, mine, origins, shapes, plane, limit)
            assert chunks[0][0] == 0 and chunks[-1][1] == len(mine)
            assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(chunks, chunks[1:] + [(len(mine),)]))
            for k_lo, k_hi, z_lo, z_hi, y_lo, y_hi in chunks:
                assert 0 <= z_lo < z_hi <= shape[0] and 0 <= y_lo < y_hi <= n_rows
                for k in range(k_lo, k_hi):
                    assert z_lo <= origins[k][0] and origins[k][0] + shapes[k][0] <= z_hi
                    assert y_lo <= origins[k][1] and origins[k][1] + shapes[k][1] <= y_hi
                inside = {coords[mine[k]][:2] for k in range(k_lo, k_hi)}
                outside = {coords[mine[k]][:2] for k in list(range(0, k_lo)) + list(range(k_hi, len(mine)))}
                box_bytes = (z_hi - z_lo) * (y_hi - y_lo) * row_bytes
                if (y_lo, y_hi) != (0, n_rows):
                    seen_cut += 1
                    assert len({c[0] for c in inside}) == 1                     # one layer
                    assert not inside & outside                                 # whole block rows
                    ys = sorted(c[1] for c in inside)
                    assert ys == list(range(ys[0], ys[-1] + 1))
                    # the box is no larger than the rows its blocks touch
                    assert y_lo == min(origins[k][1] for k in range(k_lo, k_hi))
                    assert y_hi == max(origins[k][1] + shapes[k][1] for k in range(k_lo, k_hi))
                    seen_merged += len(inside) > 1
                else:
                    assert not {c[0] for c in inside} & {c[0] for c in outside}        # whole layers
                if len(inside) > 1:
                    assert box_bytes <= limit // 2, (name, box_bytes, limit)
                elif box_bytes > limit // 2:
                    seen_oversized += 1
            every_layer_fits = all(len({coords[mine[k]][0] for k in range(c[0], c[1])}) > 1
                                   or (c[3] - c[2]) * plane <= limit // 2 for c in z_only)
            if every_layer_fits:
                assert chunks == [c + (0, n_rows) for c in z_only]
            assert every_layer_fits == (limit >= limits["layer"])
            if name == "all":
                assert len(chunks) == 1
            if name in ("row_less_one", "tiny"):
                # not even one block row of the thickest layer fits: whatever is cut is cut into single block rows
                assert all(len({coords[mine[k]][:2] for k in range(c[0], c[1])}) == 1
                           for c in chunks if (c[3] - c[2]) == max(s_[0] for s_ in shapes) and (c[4], c[5]) != (0, n_rows))
    assert seen_cut and seen_oversized
    assert seen_merged or shape[1] == 90


def test_a_share_of_one_layer_is_cut_along_y():
    """What ``_z_chunks`` alone never chunks: a stack (or a rank's share) of a single layer of blocks."""
    from magellanmapper_amd import stack_detect as sd
    shape = (30, 230, 80)
    blocks, coords = _grid(shape, 40)
    assert blocks.sub_roi_slices.shape[0] == 1 and blocks.sub_roi_slices.shape[1] == 6
    mine = list(range(len(coords)))
    origins, shapes = sd.StackDetector._block_extents(blocks.sub_roi_slices, shape, mine)
    row_bytes = shape[2] * 2
    plane = shape[1] * row_bytes
    limit = _limits(shape, origins, shapes, row_bytes)["two_rows"]
    assert sd._z_chunks(coords, mine, origins, shapes, plane, limit) == [(0, len(mine), 0, 30)]
    chunks = sd._zy_chunks(coords, mine, origins, shapes, plane, row_bytes, limit)
    # two block rows of 45 rows, 5 of them shared, per chunk: [0, 85), [80, 165), [160, 230)
    assert [c[2:] for c in chunks] == [(0, 30, 0, 85), (0, 30, 80, 165), (0, 30, 160, 230)]
    assert [c[:2] for c in chunks] == [(0, 4), (4, 8), (8, 12)]
    assert all((c[3] - c[2]) * (c[5] - c[4]) * row_bytes <= limit // 2 for c in chunks)
    # the same layer as the middle of a larger share: only that layer's chunk is cut
    assert sd._zy_chunks(coords, mine, origins, shapes, plane, row_bytes, 2 * 30 * plane) == [(0, 12, 0, 30, 0, 230)]


def test_plane_pitch_of_whole_images_boxes_and_other_views():
    """``volume._plane_pitch``: the bytes between two planes of a host array whose planes are packed -- what lets a box
    ``img[z_lo:z_hi, y_lo:y_hi]`` go up without a host copy -- and ``None`` for any other layout."""
    from magellanmapper_amd import volume
    img = np.zeros((12, 20, 16), dtype=np.uint16)
    assert volume._plane_pitch(img) == 20 * 16 * 2
    assert volume._plane_pitch(img[3:9]) == 20 * 16 * 2
    assert volume._plane_pitch(img[3:9, 4:11]) == 20 * 16 * 2            # (7 packed rows per plane, a whole plane apart)
    assert volume._plane_pitch(img[3:4, 4:11]) == 7 * 16 * 2             # (one plane: its own size)
    assert volume._plane_pitch(img[:, :, 2:9]) is None                    # rows cut: not packed
    assert volume._plane_pitch(img[::-1]) is None
    assert volume._plane_pitch(img[:, ::2]) is None
    assert volume._plane_pitch(np.broadcast_to(img[0], (4, 20, 16))) is None        # planes overlap
    two = np.zeros((6, 10, 8, 2), dtype=np.uint8)
    assert volume._plane_pitch(two[1:5, 2:7]) == 10 * 8 * 2
    assert volume._plane_pitch(two[..., 0]) is None


GRID_SHAPE, GRID_SEGMENT = (90, 230, 80), 40


def test_host_chunks_is_the_one_decision_for_a_host_image(monkeypatch):
    """``_host_chunks``: an image that fits goes up whole, as one chunk; a share of it as one chunk of the planes its
    blocks touch, every row of them; a share too large to be resident as ``_zy_chunks`` cuts it."""
    from magellanmapper_amd import stack_detect as sd
    shape = GRID_SHAPE
    blocks, coords = _grid(shape, GRID_SEGMENT)
    img = np.empty(shape, dtype=np.uint16)
    row_bytes = shape[2] * 2
    n = len(coords)
    everything = list(range(n))
    origins, shapes = sd.StackDetector._block_extents(blocks.sub_roi_slices, shape, everything)
    monkeypatch.setattr(sd, "MAX_RESIDENT_BYTES", 2 * img.nbytes)
    whole = sd._host_chunks(img, coords, everything, origins, shapes, shape)
    assert whole == [(0, n, 0, 90, 0, 230)] and whole[0].z_hi == 90 and whole[0].y_hi == 230
    # the blocks of the last two layers only: their planes, all rows
    gz = blocks.sub_roi_slices.shape[0]
    mine = [i for i in everything if coords[i][0] >= gz - 2]
    assert gz == 3 and 0 < len(mine) < n
    o2, s2 = sd.StackDetector._block_extents(blocks.sub_roi_slices, shape, mine)
    z_lo, z_hi, y_lo, y_hi = sd._share_box(o2, s2)
    assert (z_lo, z_hi, y_lo, y_hi) == (40, 90, 0, 230)
    assert sd._host_chunks(img, coords, mine, o2, s2, shape) == [(0, len(mine), z_lo, z_hi, 0, 230)]
    # the limit of tests/test_gpu_ychunks.py (_row_limit: twice the two thickest adjacent block rows of the thickest layer)
    gy = blocks.sub_roi_slices.shape[1]
    layers = [blocks.sub_roi_slices[(l, 0, 0)][0].indices(shape[0])[:2] for l in range(gz)]
    rows = [blocks.sub_roi_slices[(0, j, 0)][1].indices(shape[1])[:2] for j in range(gy)]
    limit = 2 * max(b - a for a, b in layers) * max(d[1] - c[0] for c, d in zip(rows, rows[1:])) * row_bytes
    assert limit == _limits(shape, origins, shapes, row_bytes)["two_rows"]
    monkeypatch.setattr(sd, "MAX_RESIDENT_BYTES", limit)
    want = sd._zy_chunks(coords, everything, origins, shapes, shape[1] * row_bytes, row_bytes, limit)
    assert sd._host_chunks(img, coords, everything, origins, shapes, shape) == want
    assert len(want) > 3 and any((c.y_lo, c.y_hi) != (0, 230) for c in want)
    assert all(isinstance(c, sd._Chunk) for c in want + whole)


def test_share_box_is_the_extent_of_a_shares_blocks():
    """``_share_box`` against min / max over the blocks, for a share that starts in the middle of the grid."""
    from magellanmapper_amd import stack_detect as sd
    blocks, coords = _grid(GRID_SHAPE, GRID_SEGMENT)
    mine = list(range(7, len(coords) - 5))
    assert coords[mine[0]][1:] != (0, 0) and coords[mine[0]][0] == 0
    origins, shapes = sd.StackDetector._block_extents(blocks.sub_roi_slices, GRID_SHAPE, mine)
    lo = np.asarray(origins)
    hi = lo + np.asarray(shapes)
    assert sd._share_box(origins, shapes) == (lo[:, 0].min(), hi[:, 0].max(), lo[:, 1].min(), hi[:, 1].max())
    one = [len(coords) - 1]                           # the last block alone: a box that starts inside the image
    o1, s1 = sd.StackDetector._block_extents(blocks.sub_roi_slices, GRID_SHAPE, one)
    assert sd._share_box(o1, s1) == (o1[0][0], 90, o1[0][1], 230) and o1[0][0] > 0 and o1[0][1] > 0


def _regions(nz, ny, row_bytes, cells):
    """``_SlabUpload._plan`` of an ``(nz, ny)`` image without a device: the regions in upload order."""
    from magellanmapper_amd import volume
    up = object.__new__(volume._SlabUpload)
    up.nz, up.ny, up.row_bytes = nz, ny, row_bytes
    up.slab = max(1, min(nz, volume._STREAM_CHUNK_BYTES // max(1, ny * row_bytes)))
    return up._plan(cells)


def test_chunk_cells_are_the_upload_cells_relative_to_the_box(monkeypatch):
    """``_chunk_cells``: for the whole image the ends of ``_upload_cells``; for a box every end relative to it, strictly
    inside it, ascending, the box's extent last -- and ``_SlabUpload._plan`` makes of them the very regions it made of
    the expressions the prefetch and the chunked detection each had of their own."""
    from magellanmapper_amd import stack_detect as sd, volume
    shape = GRID_SHAPE
    blocks, coords = _grid(shape, GRID_SEGMENT)
    row_bytes = shape[2] * 2
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 7 * 60 * row_bytes)      # (bands are cut along z as well)
    z_ends, y_ends = cells_all = sd._upload_cells(blocks.sub_roi_slices, shape)
    assert z_ends[-1] == 90 and y_ends[-1] == 230 and len(z_ends) == 3 and len(y_ends) == 6
    whole = sd._Chunk(0, len(coords), 0, 90, 0, 230)
    got = sd._chunk_cells(cells_all, whole)
    assert (set(got[0]), set(got[1])) == (set(z_ends), set(y_ends))
    assert _regions(90, 230, row_bytes, got) == _regions(90, 230, row_bytes, cells_all)
    assert sd._chunk_cells(None, whole) is None
    everything = list(range(len(coords)))
    origins, shapes = sd.StackDetector._block_extents(blocks.sub_roi_slices, shape, everything)
    limit = _limits(shape, origins, shapes, row_bytes)["two_rows"]
    boxes = sd._zy_chunks(coords, everything, origins, shapes, shape[1] * row_bytes, row_bytes, limit)
    boxes += [sd._Chunk(0, 1, 40, 90, 0, 230), sd._Chunk(0, 1, 3, 88, 10, 221), sd._Chunk(0, 1, 45, 46, 45, 46)]
    seen_inner = 0
    for c in boxes:
        cz, cy = sd._chunk_cells(cells_all, c)
        for ends, lo, hi in ((cz, c.z_lo, c.z_hi), (cy, c.y_lo, c.y_hi)):
            assert ends[-1] == hi - lo and all(0 < e < hi - lo for e in ends[:-1])
            assert ends == sorted(set(ends))
            assert [e + lo for e in ends[:-1]] == [e for e in (z_ends if ends is cz else y_ends) if lo < e < hi]
            seen_inner += len(ends) > 1
        # a PIN, not a reference: the expressions the chunked detection had in line before there was one helper, kept
        # here as they were -- they are the helper's body, so this only fails if the helper is edited away from them;
        # what tests the helper are the properties above
        z_lo, z_hi, y_lo, y_hi = c[2:]
        old = ([z - z_lo for z in z_ends if z_lo < z < z_hi] + [z_hi - z_lo],
               [y - y_lo for y in y_ends if y_lo < y < y_hi] + [y_hi - y_lo])
        assert _regions(z_hi - z_lo, y_hi - y_lo, row_bytes, (cz, cy)) == _regions(z_hi - z_lo, y_hi - y_lo, row_bytes, old)
        if (y_lo, y_hi) == (0, 230):
            # ... and the prefetch of a rank's planes: the z ends relative to them, the y ends of the image as they were
            old = ([z - z_lo for z in z_ends if z_lo < z < z_hi] + [z_hi - z_lo], y_ends)
            assert _regions(z_hi - z_lo, 230, row_bytes, (cz, cy)) == _regions(z_hi - z_lo, 230, row_bytes, old)
    assert seen_inner > 4
