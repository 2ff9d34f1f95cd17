"""The blur and the rotation behind the training augmentation, host side (no GPU): the rule of asy-vrnet_amd/data.py pinned
to things that are not the rule -- scipy's mirror correlation for the blur, the partition of unity and the identity for the
cubic weights, a linear ramp (which every cubic kernel reproduces) for the rotated canvas, a drawn box for the agreement of
`rotate_nearest` with `rotate_boxes`, and the generator's state for the draw."""
import numpy as np
import pytest
import scipy.ndimage as ndi

from asy_vrnet_amd import data


# ---- the blur -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8), (9, 13), (40, 63)])
def test_blur_equals_scipys_mirror_correlation_applied_twice(shape):
    a = np.random.default_rng(shape[1]).integers(0, 256, shape + (3,), dtype=np.uint8)
    w = np.array([1, 4, 6, 4, 1], np.int64)
    s = ndi.correlate1d(ndi.correlate1d(a.astype(np.int64), w, axis=0, mode="mirror"), w, axis=1, mode="mirror")
    got = data.gaussian_blur5_u8(a)
    assert got.dtype == np.uint8 and np.array_equal(got, ((s + 128) >> 8).astype(np.uint8))
    assert (got != a).any()


def test_blur_leaves_a_constant_canvas_unchanged():
    for v in (0, 1, 128, 255):
        a = np.full((9, 13, 3), v, np.uint8)
        assert np.array_equal(data.gaussian_blur5_u8(a), a)
    with pytest.raises(RuntimeError, match="H, W >= 3"):
        data.gaussian_blur5_u8(np.zeros((2, 9, 3), np.uint8))


# ---- the cubic weights ----------------------------------------------------------------------------------------------------
def test_all_1024_weight_sets_sum_to_32768_and_0_0_is_the_identity():
    ay, ax = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    wt = data.cubic_weights(ay, ax)
    assert wt.shape == (32, 32, 4, 4) and wt.dtype == np.int32
    assert (wt.reshape(1024, 16).sum(1) == 32768).all()
    want = np.zeros((4, 4), np.int32)
    want[1, 1] = 32768
    assert np.array_equal(wt[0, 0], want) and np.array_equal(data.cubic_weights(0, 0), want)
    # the coefficients are a partition of unity in float32 up to rounding, and symmetric: c(t)[k] = c(1 - t)[3 - k]
    c = data.cubic_coeffs(np.arange(32))
    assert c.dtype == np.float32 and np.abs(c.sum(1) - 1).max() < 1e-6
    assert np.abs(c[1:] - c[1:][::-1, ::-1]).max() < 1e-6
    # a set whose sum had to be mended differs from the plain rounding in one central weight only
    f32 = np.float32
    plain = np.rint((c[:, None, :, None] * c[None, :, None, :]).astype(f32) * f32(32768)).astype(np.int32)
    assert np.abs(32768 - plain.reshape(1024, 16).astype(np.int64).sum(1)).max() <= 8
    changed = (plain != wt)
    assert changed.any() and changed.reshape(1024, 16).sum(1).max() == 1 and not changed[..., [0, 3], :].any() and \
        not changed[..., :, [0, 3]].any()


# ---- angle 0 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64), (40, 63)])
def test_angle_0_is_the_identity(shape):
    rng = np.random.default_rng(7)
    fwd, inv = data.rotation_matrices(shape, 0)
    canvas = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    plane = rng.standard_normal(shape).astype(np.float32)
    assert np.array_equal(data.rotate_canvas_u8(canvas, inv), canvas)
    assert np.array_equal(data.rotate_nearest(canvas[..., 0], inv, 0), canvas[..., 0])
    assert data.rotate_nearest(plane, inv, 0.0).tobytes() == plane.tobytes()
    box = np.array([[3, 5, 41, 33, 0], [0, 0, shape[1], shape[0], 2]], np.int64)
    assert np.array_equal(data.rotate_boxes(box.copy(), fwd, shape[1], shape[0]), box)
    rec = data.aug_post_record(shape, False, 0)
    assert int(rec["rotate"]) == 0 and int(rec["blur"]) == 0


def test_the_inverse_matrix_inverts_the_forward_one():
    for angle in (10, -10, 3):
        fwd, inv = data.rotation_matrices((40, 63), angle)
        F = np.vstack([fwd.reshape(2, 3), [0, 0, 1]])
        I = np.vstack([inv.reshape(2, 3), [0, 0, 1]])
        assert np.abs(F @ I - np.eye(3)).max() < 1e-12
        # the centre (W // 2, H // 2) is the fixed point
        assert np.abs(F @ [31, 20, 1] - [31, 20, 1]).max() < 1e-12
    # the reference passes -rotation to getRotationMatrix2D: its positive angle turns the image clockwise on the screen
    fwd = data.rotation_matrices((64, 64), 10)[0]
    assert fwd[1] < 0 < fwd[3]


# ---- the rotated canvas on a linear ramp ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [10, -10])
def test_rotated_ramp_equals_the_ramp_at_the_inverse_coordinate(angle):
    """Every cubic kernel reproduces a linear function of the coordinates, so on canvas[y, x] = gx x + gy y + c (whole
    numbers, no byte clipped) the rotated canvas is the ramp at the source coordinate the walk stands for.  The walk keeps the
    coordinate on a 1 / 32 grid: X = (rint(1024 u) + 16) >> 5 with u the float64 inverse coordinate, after two roundings to
    1 / 1024 (adelta and X0, half a unit each), so |X / 32 - u| <= 1 / 64 + 1 / 1024 per axis.  The sixteen integer weights
    differ from the exact products by at most half a unit of 2^-15 each before the sum is mended by |diff| <= 8 units on one
    weight, and every tap is at most 255: below 16 * 0.5 * 255 / 32768 + 8 * 255 / 32768 < 0.13 of a level.  The float32
    coefficients add less than 1e-4.  The final rounding adds half a level.  Bound: (|gx| + |gy|) (1 / 64 + 1 / 1024) + 0.13
    + 0.5, rounded up to whole levels since both sides are integers.  Pixels whose 4 x 4 taps touch the border are left out."""
    H, W, gx, gy, c0 = 64, 64, 2, 1, 30
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = gx * xx + gy * yy + c0
    assert ramp.min() >= 0 and ramp.max() <= 255
    canvas = np.repeat(ramp.astype(np.uint8)[..., None], 3, -1)
    inv = data.rotation_matrices((H, W), angle)[1]
    got = data.rotate_canvas_u8(canvas, inv).astype(np.int64)
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()
    u = inv[0] * xx + inv[1] * yy + inv[2]
    v = inv[3] * xx + inv[4] * yy + inv[5]
    sx, sy, _, _ = data.warp_coords(inv, H, W, False)
    inner = (sx - 1 >= 0) & (sx + 2 <= W - 1) & (sy - 1 >= 0) & (sy + 2 <= H - 1)
    assert inner.sum() > 0.6 * H * W
    bound = int(np.ceil((abs(gx) + abs(gy)) * (1 / 64 + 1 / 1024) + 0.13 + 0.5))
    want = gx * u + gy * v + c0
    err = np.abs(got[..., 0] - want)[inner]
    print("ramp: max error", err.max(), "bound", bound)
    assert err.max() <= bound
    # the grid claim itself
    _, _, ax, ay = data.warp_coords(inv, H, W, False)
    assert np.abs(sx + ax / 32 - u).max() <= 1 / 64 + 1 / 1024 and np.abs(sy + ay / 32 - v).max() <= 1 / 64 + 1 / 1024
    # outside the rotated canvas the border is grey
    assert tuple(got[0, 0]) == (128, 128, 128) or tuple(got[0, W - 1]) == (128, 128, 128)


# ---- the label map and the boxes agree -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [10, -10])
def test_the_centre_of_a_drawn_box_lands_inside_the_rotated_box(angle):
    H = W = 64
    fwd, inv = data.rotation_matrices((H, W), angle)
    for x1, y1, x2, y2 in ((10, 12, 30, 40), (40, 8, 58, 20), (2, 44, 25, 60), (28, 28, 36, 36)):
        label = np.zeros((H, W), np.uint8)
        label[y1:y2, x1:x2] = 1
        rot = data.rotate_nearest(label, inv, 0)
        assert rot.dtype == np.uint8 and rot.sum() > 0.5 * label.sum()
        ys, xs = np.nonzero(rot)
        box = data.rotate_boxes(np.array([[x1, y1, x2, y2, 1]], np.int64), fwd, W, H)[0]
        # the centre of mass of the rotated region is inside the rotated box, and the region inside the box's rows and columns
        assert box[0] <= xs.mean() <= box[2] and box[1] <= ys.mean() <= box[3]
        assert box[0] - 1 <= xs.min() and xs.max() <= box[2] + 1 and box[1] - 1 <= ys.min() and ys.max() <= box[3] + 1
        # the box's own centre goes to the rotated box's centre, up to the truncation of its corners
        cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
        rx, ry = fwd[0] * cx + fwd[1] * cy + fwd[2], fwd[3] * cx + fwd[4] * cy + fwd[5]
        assert abs(rx - (box[0] + box[2]) / 2) <= 1 and abs(ry - (box[1] + box[3]) / 2) <= 1
        assert rot[int(round(ry)), int(round(rx))] == 1
    # fill: outside the rotated canvas the label is 0 and the radar 0.0
    ones = data.rotate_nearest(np.ones((H, W), np.float32), inv, 0.0)
    assert ones.dtype == np.float32 and set(np.unique(ones).tolist()) == {0.0, 1.0} and ones[H // 2, W // 2] == 1.0


def test_augment_boxes_without_a_rotation_is_unchanged_and_clips_once_behind_it():
    rec = data.aug_record((48, 80), (64, 64), 100, 70, -20, -3, True, False)
    boxes = np.array([[3, 5, 41, 33, 0], [10, 0, 12, 40, 1], [50, 20, 200, 100, 3], [-20, -30, 30, 30, 0]])
    plain = data.augment_boxes(boxes, 80, 48, 64, 64, rec)
    assert np.array_equal(plain, data.augment_boxes(boxes, 80, 48, 64, 64, rec, data.aug_post_record((64, 64), True, 0)))
    post = data.aug_post_record((64, 64), False, 10)
    rot = data.augment_boxes(boxes, 80, 48, 64, 64, rec, post)
    assert rot.dtype == np.float64 and len(rot) and (rot[:, :4] >= 0).all() and (rot[:, [0, 2]] <= 64).all() and (rot[:, [1, 3]] <= 64).all()
    assert not np.array_equal(rot, plain)
    # the rotation runs on the UNCLIPPED rows: rotating the clipped ones gives other boxes
    clipped = data.rotate_boxes(plain.astype(np.int64), post["fwd"], 64, 64)
    assert not np.array_equal(clipped[:, :4].clip(0, 64), rot[:, :4])


# ---- the draw and the record ------------------------------------------------------------------------------------------------------
def test_the_record_is_112_bytes():
    assert data.AUG_POST_DTYPE.itemsize == 112
    assert [data.AUG_POST_DTYPE.fields[k][1] for k in ("blur", "rotate", "angle", "reserved", "inv", "fwd")] == [0, 4, 8, 12, 16, 64]
    tab = data.augment_post_params(3, (64, 64), 0, 1.0, 1.0)
    assert tuple(data.aug_post_bytes(tab).shape) == (3, 112)


def test_with_both_probabilities_0_the_generator_is_where_augment_params_leaves_it():
    sizes = [(48, 80), (90, 60)]
    r1, r2 = np.random.RandomState(11), np.random.RandomState(11)
    t1 = data.augment_params(sizes, (64, 64), r1)
    t2 = data.augment_params(sizes, (64, 64), r2)
    post = data.augment_post_params(2, (64, 64), r2, blur=0, rotate=0)
    assert t1.tobytes() == t2.tobytes() and r1.rand() == r2.rand()
    assert not post["blur"].any() and not post["rotate"].any() and not post["angle"].any()
    # with one of them on, three values per image are drawn, in the order blur, rotate, angle, always all three
    r3, r4 = np.random.RandomState(5), np.random.RandomState(5)
    post = data.augment_post_params(4, (64, 64), r3, blur=.25, rotate=0)
    want = []
    for _ in range(4):
        want.append((int(r4.rand() < .25), int(r4.rand() < 0), r4.randint(-10, 11)))
    assert r3.rand() == r4.rand()
    assert [int(b) for b in post["blur"]] == [w[0] for w in want] and not post["rotate"].any() and not post["angle"].any()
    # a drawn angle of 0 is no rotation; an angle is kept only with its rotation
    post = data.augment_post_params(64, (64, 64), 1, blur=1, rotate=1, max_angle=1)
    assert set(post["angle"].tolist()) == {-1, 0, 1} and ((post["angle"] != 0) == (post["rotate"] == 1)).all() and post["blur"].all()
    for t in post:
        fwd, inv = data.rotation_matrices((64, 64), int(t["angle"]))
        assert t["fwd"].tobytes() == fwd.tobytes() and t["inv"].tobytes() == inv.tobytes()


def test_a_bad_post_record_is_rejected_by_name():
    tab = data.augment_post_params(3, (64, 64), 0, 1.0, 1.0)
    assert data.check_aug_post_table(tab, (64, 64), 10, 3) is not None
    bad = tab.copy()
    bad[1]["inv"][2] = np.nan
    with pytest.raises(RuntimeError, match="image 1.*not finite"):
        data.check_aug_post_table(bad, (64, 64), 10)
    bad = tab.copy()
    bad[2]["fwd"][0] = np.inf
    with pytest.raises(RuntimeError, match="image 2.*not finite"):
        data.check_aug_post_table(bad, (64, 64), 10)
    bad = tab.copy()
    bad[0] = data.aug_post_record((64, 64), False, -11)
    with pytest.raises(RuntimeError, match="image 0.*angle -11.*max_angle = 10"):
        data.check_aug_post_table(bad, (64, 64), 10)
    with pytest.raises(RuntimeError, match="AUG_POST_DTYPE"):
        data.check_aug_post_table(tab, (64, 64), 10, batch=2)
    with pytest.raises(RuntimeError, match="at least 8 x 8"):
        data.check_aug_post_table(tab, (7, 64), 10)


def test_augment_sample_without_a_post_record_returns_what_it_returned():
    from PIL import Image
    rng = np.random.default_rng(3)
    frame, label = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8), rng.integers(0, 6, (48, 80), dtype=np.uint8)
    radar = rng.standard_normal((4, 64, 64)).astype(np.float32)
    boxes = np.array([[3, 5, 41, 33, 0], [50, 20, 200, 100, 3]])
    rec = data.aug_record((48, 80), (64, 64), 100, 70, -20, -3, True, True, (1.05, 1.3, 0.8))
    plain = data.augment_sample(Image.fromarray(frame), Image.fromarray(label), boxes, radar, (64, 64), rec)
    ident = data.augment_sample(Image.fromarray(frame), Image.fromarray(label), boxes, radar, (64, 64), rec,
                                post=data.aug_post_record((64, 64), False, 0))
    for a, b in zip(plain, ident):
        assert np.array_equal(np.array(a), np.array(b))
    both = data.augment_sample(Image.fromarray(frame), Image.fromarray(label), boxes, radar, (64, 64), rec,
                               post=data.aug_post_record((64, 64), True, -10))
    assert (np.array(both[0]) != np.array(plain[0])).any() and (np.array(both[2]) != np.array(plain[2])).any()
    assert (both[3] != plain[3]).any() and both[3].dtype == np.float32
    # the order: the colour stage runs behind the rotation, so the grey border of the rotation is recoloured with the rest
    corner = tuple(np.array(both[0])[0, 0])
    assert corner == tuple(data.hsv_jitter(np.full((1, 1, 3), 128, np.uint8), rec["lut"])[0, 0])
