"""The host side of training from raw frames (no GPU): `data.pack_boxes`, and the decode-only `data.FrameDataset` with
`data.frames_collate` on three tiny files written with Pillow and numpy."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from asy_vrnet_amd import data


def test_pack_boxes_layout_and_errors():
    boxes = [np.array([[1, 2, 30, 40, 3], [-5, 0, 7, 9, 0]]), None, np.zeros((0, 5), np.int64), torch.tensor([[4, 5, 6, 7, 1]])]
    packed, counts = data.pack_boxes(boxes, 3)
    assert packed.dtype == torch.int32 and tuple(packed.shape) == (4, 3, 5) and not packed.is_cuda
    assert counts.dtype == torch.int32 and counts.tolist() == [2, 0, 0, 1]
    assert packed.is_pinned() == counts.is_pinned() == torch.cuda.is_available()
    assert packed[0, :2].tolist() == [[1, 2, 30, 40, 3], [-5, 0, 7, 9, 0]] and packed[3, 0].tolist() == [4, 5, 6, 7, 1]
    assert not packed[0, 2:].any() and not packed[1].any() and not packed[2].any() and not packed[3, 1:].any()
    full, n = data.pack_boxes([np.ones((3, 5), np.int32)], 3)                    # exactly max_gt rows
    assert n.tolist() == [3] and full.eq(1).all()
    empty, n = data.pack_boxes([None, []], 0)                                    # max_gt = 0 keeps one (unused) row
    assert tuple(empty.shape) == (2, 1, 5) and n.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="image 1 has 4 boxes, above max_gt = 3"):
        data.pack_boxes([boxes[0], np.ones((4, 5), np.int64)], 3)
    with pytest.raises(RuntimeError, match="image 2.*integer"):
        data.pack_boxes([None, None, np.array([[1.0, 2.0, 3.0, 4.0, 0.0]])], 3)
    with pytest.raises(RuntimeError, match="image 0.*integer"):
        data.pack_boxes([torch.ones(1, 5)], 3)
    with pytest.raises(RuntimeError, match=r"image 0.*\(n, 5\)"):
        data.pack_boxes([np.ones((2, 4), np.int64)], 3)
    with pytest.raises(RuntimeError, match="image 0.*int32"):
        data.pack_boxes([np.array([[0, 0, 2 ** 31, 5, 0]])], 3)


FIDS = ["1664091257.87023", "1664091300.00001", "1664099999.12345"]
SIZES = [(30, 52), (47, 33), (40, 40)]
TAILS = ["3,4,30,20,1 -5,2,12,29,0", "", "0,0,40,40,2"]


@pytest.fixture()
def files(tmp_path):
    rng = np.random.default_rng(3)
    seg, radar = tmp_path / "seg", tmp_path / "radar"
    os.makedirs(seg / "VOC2007" / "SegmentationClass")
    os.makedirs(radar)
    os.makedirs(tmp_path / "0000000000.00000")                # an earlier match in the path: the LAST one names the frame
    lines, want = [], []
    for fid, (ih, iw), tail in zip(FIDS, SIZES, TAILS):
        frame = rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
        label = rng.integers(0, 12, (ih, iw), dtype=np.uint8)
        maps = rng.standard_normal((4, 16, 16))                # float64 on disk, as np.savez stores it
        path = str(tmp_path / "0000000000.00000" / (fid + ".png"))        # lossless, so the decoded bytes are known
        Image.fromarray(frame).save(path)
        Image.fromarray(label).save(str(seg / "VOC2007" / "SegmentationClass" / (fid + ".png")))
        np.savez(radar / (fid + ".npz"), maps)
        lines.append(path + (" " + tail if tail else ""))
        want.append((frame, maps, label))
    return data.FrameDataset(lines, str(seg), str(radar)), lines, want


def test_frame_dataset_decodes_and_nothing_more(files):
    ds, lines, want = files
    assert len(ds) == 3
    for i, (line, (frame, maps, label)) in enumerate(zip(lines, want)):
        assert data.frame_id(line) == FIDS[i]                                  # dataloader.py:73-76
        f, r, boxes, l, size = ds[i]
        assert f.dtype == np.uint8 and np.array_equal(f, frame) and l.dtype == np.uint8 and np.array_equal(l, label)
        assert r.dtype == np.float32 and np.array_equal(r, maps.astype(np.float32))
        assert tuple(size) == SIZES[i] == f.shape[:2] == l.shape
        assert boxes.dtype == np.int64 and np.array_equal(boxes, data.parse_annotation_line(line)[1])
    assert ds[1][2].shape == (0, 5) and ds[0][2].tolist() == [[3, 4, 30, 20, 1], [-5, 2, 12, 29, 0]]
    assert np.array_equal(ds[4][0], want[1][0])                                # index % length, dataloader.py:71


def test_frame_dataset_rejects_a_label_map_of_another_size(files):
    ds, lines, want = files
    Image.fromarray(want[0][2][:-1]).save(os.path.join(ds.seg_dataset_path, "VOC2007/SegmentationClass", FIDS[0] + ".png"))
    with pytest.raises(RuntimeError, match="label map"):
        ds[0]


def test_frames_collate_returns_the_arguments_of_the_step(files):
    ds, lines, want = files
    loader = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False, collate_fn=data.frames_collate)
    (frames, radar, boxes, labels, sizes), = list(loader)
    assert radar.dtype == torch.float32 and tuple(radar.shape) == (3, 4, 16, 16)
    assert sizes.dtype == np.int64 and sizes.tolist() == [list(s) for s in SIZES]
    assert [tuple(f.shape) for f in frames] == [s + (3,) for s in SIZES] and all(f.dtype == torch.uint8 for f in frames)
    assert [tuple(l.shape) for l in labels] == SIZES and all(l.dtype == torch.uint8 for l in labels)
    # the batch is what the ragged entry points validate and pack
    items, own = data.ragged_items(frames, sizes, 3, (3,), "frames", "test")
    labs, _ = data.ragged_items(labels, own, 3, (), "label maps", "test")
    assert own.tolist() == sizes.tolist() and all(torch.equal(a, b) for a, b in zip(items, frames)) and len(labs) == 3
    packed, counts = data.pack_boxes(boxes, 4)
    assert counts.tolist() == [2, 0, 1] and packed[2, 0].tolist() == [0, 0, 40, 40, 2]
    table = data.frame_geometry(own, (32, 32), True, (47, 52))
    assert table["ih"].tolist() == [30, 47, 40] and table["iw"].tolist() == [52, 33, 40]
