"""CPU: the by-value tables of the one-call matcher and of the staging-free pseudo-label chain -- their sizes against the limit
the header documents, what the built kernels really take as arguments, the packing of 0, 1 and the maximum number of problems,
and the host-side refusals of the new entry points (no GPU needed: every check comes before the first launch)."""
import ctypes
import os
import re

import pytest

from semi_detr_amd import _lib, matcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "semidetr_hip.h")).read()
KERNARG_LIMIT = 4096          # bytes of kernel arguments one HIP launch accepts, as the header states it


def _macro(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, HEADER).group(1))


def test_table_sizes_are_the_documented_ones_and_fit_the_kernel_arguments():
    assert _macro("SEMIDETR_MATCH_TABLE") == _lib.MATCH_TABLE >= 35          # a warm-up loss() call has 35 problems, the benchmark 28
    assert _macro("SEMIDETR_IMAGE_TABLE") == _lib.IMAGE_TABLE
    assert "of the 4096" in HEADER
    for struct, cls in (("semidetr_match_table", _lib.MatchTable), ("semidetr_image_sizes", _lib.ImageSizes),
                        ("semidetr_box_table", _lib.BoxTable)):
        documented = int(re.search(r"sizeof\(%s\) = (\d+)" % struct, HEADER).group(1))
        assert ctypes.sizeof(cls) == documented
        assert documented + 128 <= KERNARG_LIMIT            # the other arguments of the kernels that carry it: below 128 bytes


def test_built_kernels_take_the_tables_in_their_arguments():
    from test_cabi_host import _code_object_kernels
    meta = _code_object_kernels(_lib.LIB_PATH)
    sizes = {n: k[".kernarg_segment_size"] for n, k in meta.items()}
    assert max(sizes.values()) <= KERNARG_LIMIT
    table = {n: s for n, s in sizes.items() if "TableGt" in n or "TableBoxes" in n or "ValueHw" in n}
    assert {n.split("<")[0] for n in table} == {"match_cost_kernel", "lsap_kernel", "build_targets_kernel", "nms_prepare_kernel",
                                                "transform_bboxes_kernel"}
    documented = int(re.search(r"the assignment's\) is (\d+) bytes", HEADER).group(1))
    for n, s in table.items():         # the whole table is in the argument block, and nothing of it went to scratch
        assert s > ctypes.sizeof(_lib.ImageSizes) and meta[n][".private_segment_fixed_size"] == 0, n
    assert max(s for n, s in table.items() if n.startswith("lsap_kernel")) == documented


def test_packing_zero_one_and_the_maximum_number_of_problems():
    T = _lib.MATCH_TABLE
    for bad in (0, T + 1):
        with pytest.raises(ValueError, match="fit the table"):
            matcher.pack_match_table([16] * bad, [8] * bad, [1] * bad, [(4, 3)] * bad)
    with pytest.raises(ValueError):
        matcher.pack_match_table([16], [8, 8], [1], [(4, 3)])
    t, offs = matcher.pack_match_table([4096], [8192], [7], [(1333, 800)])
    assert (t.num_problems, t.count[0], t.offsets[0], t.offsets[1], t.boxes[0], t.labels[0]) == (1, 7, 0, 7, 4096, 8192)
    assert (t.img_wh[0][0], t.img_wh[0][1]) == (1333.0, 800.0) and offs == [0, 7] and t.boxes[1] is None and t.count[1] == 0
    counts = [b % 17 for b in range(T)]
    t, offs = matcher.pack_match_table([16 * (b + 1) for b in range(T)], [0 if c == 0 else 8 * (b + 1) for b, c in enumerate(counts)],
                                       counts, [(100 + b, 50 + b) for b in range(T)])
    assert t.num_problems == T and list(t.count) == counts and list(t.offsets) == offs and len(offs) == T + 1
    assert offs[-1] == sum(counts) and all(offs[b + 1] - offs[b] == counts[b] for b in range(T))
    assert [t.boxes[b] for b in range(T)] == [16 * (b + 1) for b in range(T)]
    assert [t.labels[b] or 0 for b in range(T)] == [0 if c == 0 else 8 * (b + 1) for b, c in enumerate(counts)]
    assert [(t.img_wh[b][0], t.img_wh[b][1]) for b in range(T)] == [(100.0 + b, 50.0 + b) for b in range(T)]


def test_the_entry_points_refuse_bad_tables_on_the_host():
    lib = _lib.lib()
    prm = _lib.CostParams(2.0, 0.25, 2.0, 1e-12, 5.0, 1, 2.0, 1, 0)

    def assign(table, cost=4096, status=4096):
        return lib.semidetr_hungarian_assign_f32(None, 4096, 4096, ctypes.byref(table), 8, 3, ctypes.byref(prm), cost, None, None,
                                                 4096, 4096, status, None, 0, None, None, None, None, None)
    empty = _lib.MatchTable()
    assert assign(empty) == -1 and b"fit the table" in lib.semidetr_last_error()
    t, _ = matcher.pack_match_table([4096, 8192], [4096, 8192], [3, 2], [(10, 10)] * 2)
    t.offsets[1] = 4
    assert assign(t) == -1 and b"offset 4" in lib.semidetr_last_error()
    t, _ = matcher.pack_match_table([4096, 8196], [4096, 8192], [3, 2], [(10, 10)] * 2)
    assert assign(t) == -1 and b"aligned" in lib.semidetr_last_error()
    t, _ = matcher.pack_match_table([4096, 0], [4096, 8192], [3, 2], [(10, 10)] * 2)
    assert assign(t) == -1 and b"null boxes" in lib.semidetr_last_error()
    t, _ = matcher.pack_match_table([4096, 8192], [4096, 8192], [3, 2], [(10, 10)] * 2)
    assert assign(t, status=None) == -1 and b"null status" in lib.semidetr_last_error()
    assert assign(t, cost=None) == -1 and b"null pointer" in lib.semidetr_last_error()
    with pytest.raises(ctypes.ArgumentError):          # a block of another op is refused before anything runs
        lib.semidetr_hungarian_assign_f32(None, 4096, 4096, ctypes.byref(_lib.BoxTable()), 8, 3, ctypes.byref(prm), 4096, None, None,
                                          4096, 4096, 4096, None, 0, None, None, None, None, None)
    boxes = _lib.BoxTable()
    assert lib.semidetr_transform_bboxes_table_f32(None, ctypes.byref(boxes), 4096) == -1
    boxes.num_images, boxes.count[0], boxes.box_stride[0] = 1, 5, 4
    assert lib.semidetr_transform_bboxes_table_f32(None, ctypes.byref(boxes), 4096) == -1 and b"null boxes" in lib.semidetr_last_error()
    boxes.count[0] = 0                                 # nothing to warp: no launch, no error
    assert lib.semidetr_transform_bboxes_table_f32(None, ctypes.byref(boxes), None) == 0
    sizes = _lib.ImageSizes()
    args = (8, 3, 0.01, 0.6, 300, 4096, 1 << 20, 4096, 4096, 4096, 4096, 4096, 4096, 4096)
    assert lib.semidetr_teacher_pseudo_labels_f32(None, 4096, 4096, ctypes.byref(sizes), *args) == -1
    assert b"fit the table" in lib.semidetr_last_error()
    sizes.num_images = _lib.IMAGE_TABLE + 1
    assert lib.semidetr_teacher_pseudo_labels_f32(None, 4096, 4096, ctypes.byref(sizes), *args) == -1
