"""vr_transform_u8 (csrc/transform.hip) at the edges tests/test_transform.py never reaches,
against Pillow itself (the _pil_ref pipeline of tests/test_transform.py), bit for bit:
crops wider than one 256-thread column block, the 63-tap limit and the 65-tap refusal,
sums that clamp on both sides in both passes, half-to-even crop offsets that round up,
one-pixel and identity axes, the C entry point's refusals / workspace bounds, and the
ToTensor-only path of DeviceTransform.

The premises of the GPU cases -- resized size, unrounded crop offsets, tap counts, that the
hard-edge images really drive the sums outside [0, 255] -- are asserted without a GPU on the
very images and settings the GPU tests use (the pattern of tests/test_full_edges_keys.py),
and the numpy oracle is pinned to Pillow on every one of them.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest

from oracle import transform_oracle as T
from test_transform import _img, _pil_ref

# how: the public constructor that expresses the setting, or None for a direct
#      DeviceTransform(resize, crop, imgnet mean, imgnet std, interpolation=kind)
# nhw: resized (height, width); offs: (top, left) before rounding; taps: (horizontal, vertical)
Case = namedtuple("Case", "name hw how resize crop kind nhw offs taps")

# item 2: crops beyond one 256-thread column block
BLOCK_CASES = [
    Case("clip336-425x425", (425, 425), "clip336", 336, 336, "bicubic", (336, 336), (0.0, 0.0), (7, 7)),
    Case("clip336-300x500", (300, 500), "clip336", 336, 336, "bicubic", (336, 560), (0.0, 112.0), (5, 5)),
    Case("clip336-500x300", (500, 300), "clip336", 336, 336, "bicubic", (560, 336), (112.0, 0.0), (5, 5)),
    Case("clip336-336x400-identity-rows", (336, 400), "clip336", 336, 336, "bicubic", (336, 400), (0.0, 32.0),
         (5, 5)),
    Case("clip336-64x90-upscale", (64, 90), "clip336", 336, 336, "bicubic", (336, 472), (0.0, 68.0), (5, 5)),
    Case("crop513-three-blocks", (300, 420), None, 600, 513, "bilinear", (600, 840), (43.5, 163.5), (3, 3)),
    Case("crop257-one-live-column", (300, 420), None, 257, 257, "bilinear", (257, 359), (0.0, 51.0), (5, 5)),
    Case("crop256-full-block", (300, 420), None, 256, 256, "bilinear", (256, 358), (0.0, 51.0), (5, 5)),
    Case("dino518", (300, 420), "dino518", 518, 518, "bicubic", (518, 725), (0.0, 103.5), (5, 5)),
]

# item 3: crop placement and degenerate geometry
PLACE_CASES = [
    Case("left-59.5-up", (256, 343), "imgnet", 256, 224, "bilinear", (256, 343), (16.0, 59.5), (3, 3)),
    Case("top-59.5-up", (343, 256), "imgnet", 256, 224, "bilinear", (343, 256), (59.5, 16.0), (3, 3)),
    Case("crop1", (300, 420), None, 256, 1, "bilinear", (256, 358), (127.5, 178.5), (5, 5)),
    Case("crop255", (300, 420), None, 256, 255, "bilinear", (256, 358), (0.5, 51.5), (5, 5)),
    Case("1x1", (1, 1), "imgnet", 256, 224, "bilinear", (256, 256), (16.0, 16.0), (3, 3)),
    Case("1x7", (1, 7), "imgnet", 256, 224, "bilinear", (256, 1792), (16.0, 784.0), (3, 3)),
    Case("7x1-bicubic", (7, 1), None, 256, 224, "bicubic", (1792, 256), (784.0, 16.0), (5, 5)),
    Case("2x3-bicubic", (2, 3), None, 64, 64, "bicubic", (64, 96), (0.0, 16.0), (5, 5)),
    Case("clip-224x300-identity-rows", (224, 300), "clip", 224, 224, "bicubic", (224, 300), (0.0, 38.0), (5, 5)),
    Case("tiny-300x500", (300, 500), "tiny-imagenet", 64, 64, "bilinear", (64, 106), (0.0, 21.0), (11, 11)),
]

# item 4: hard-edge images (the four patterns of PATTERNS share a launch)
SAT_CASES = [
    Case("sat-imgnet-300x420", (300, 420), "imgnet", 256, 224, "bilinear", (256, 358), (16.0, 67.0), (5, 5)),
    Case("sat-imgnet-64x90", (64, 90), "imgnet", 256, 224, "bilinear", (256, 360), (16.0, 68.0), (3, 3)),
    Case("sat-clip-300x420", (300, 420), "clip", 224, 224, "bicubic", (224, 313), (0.0, 44.5), (7, 7)),
    Case("sat-clip-64x90", (64, 90), "clip", 224, 224, "bicubic", (224, 315), (0.0, 45.5), (5, 5)),
]
PATTERNS = ["checker2", "stripes3", "all0", "all255"]

# item 5: the tap limit; 63 taps is the widest accepted window (ksize is odd), 65 is refused
TAP_OK_CASES = [
    Case("taps63-248x248", (248, 248), None, 8, 8, "bilinear", (8, 8), (0.0, 0.0), (63, 63)),
    Case("taps63-248x496", (248, 496), None, 8, 8, "bilinear", (8, 16), (0.0, 4.0), (63, 63)),
    Case("taps63-124x124-bicubic", (124, 124), None, 8, 8, "bicubic", (8, 8), (0.0, 0.0), (63, 63)),
    Case("taps63-124x248-bicubic-crop5", (124, 248), None, 8, 5, "bicubic", (8, 16), (1.5, 5.5), (63, 63)),
]
TAP_REFUSED_CASES = [
    Case("taps65-249x249", (249, 249), None, 8, 8, "bilinear", (8, 8), (0.0, 0.0), (65, 65)),
    Case("taps65-125x125-bicubic", (125, 125), None, 8, 8, "bicubic", (8, 8), (0.0, 0.0), (65, 65)),
    Case("taps65-horizontal-only", (248, 250), None, 8, 8, "bilinear", (8, 8), (0.0, 0.0), (65, 63)),
]

ALL_CASES = BLOCK_CASES + PLACE_CASES + SAT_CASES + TAP_OK_CASES + TAP_REFUSED_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# the three launches of the C entry point's guard test: one of item 2, one of item 5, (1, 7)
GUARD_CASES = [BY_NAME["crop513-three-blocks"], BY_NAME["taps63-124x248-bicubic-crop5"], BY_NAME["1x7"]]

_ids = lambda cases: [c.name for c in cases]  # noqa: E731


def _stats(case):
    """(mean, std) the case's transform normalises with."""
    from visreps_amd.dataloaders.obj_cls import DS_MEAN, DS_STD

    if case.how in ("clip", "clip336"):
        from visreps_amd.models.foundation import CLIP_MEAN, CLIP_STD

        return CLIP_MEAN, CLIP_STD
    key = "tiny-imagenet" if case.how == "tiny-imagenet" else "imgnet"
    return DS_MEAN[key], DS_STD[key]


def _tf(case):
    from visreps_amd.dataloaders.obj_cls import (DeviceTransform, clip_transform, dino_transform,
                                                 get_transform)

    if case.how in ("imgnet", "tiny-imagenet"):
        return get_transform(case.how)
    if case.how == "clip":
        return clip_transform()
    if case.how == "clip336":
        return clip_transform(336)
    if case.how == "dino518":
        return dino_transform(518)
    assert case.how is None
    mean, std = _stats(case)
    return DeviceTransform(case.resize, case.crop, mean, std, interpolation=case.kind)


def _pattern(name, h, w):
    """Hard-edge image: channels (a, 255 - a, a) of a 0/255 field a."""
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "checker2":
        a = ((yy // 2 + xx // 2) % 2) * 255
    elif name == "stripes3":
        a = (xx % 3 == 0) * 255
    else:
        a = np.full((h, w), {"all0": 0, "all255": 255}[name])
    a = a.astype(np.uint8)
    return np.ascontiguousarray(np.stack([a, 255 - a, a], axis=2))


@functools.lru_cache(maxsize=None)
def _images(name):
    """The case's batch: B = 2 seeded images of different content, or the four patterns."""
    case = BY_NAME[name]
    h, w = case.hw
    if case in SAT_CASES:
        imgs = [_pattern(p, h, w) for p in PATTERNS]
    else:
        seed = 1000 + 2 * ALL_CASES.index(case)
        # _img's arrays are not C-contiguous; the C entry point is handed these bytes as they lie
        imgs = [np.ascontiguousarray(_img(h, w, seed)), np.ascontiguousarray(_img(h, w, seed + 1))]
    for im in imgs:
        im.setflags(write=False)
    return tuple(imgs)


@functools.lru_cache(maxsize=None)
def _refs(name):
    """Pillow's result for every image of the case, computed once and left unchanged."""
    case = BY_NAME[name]
    mean, std = _stats(case)
    refs = [_pil_ref(im, case.resize, case.crop, mean, std, case.kind) for im in _images(name)]
    for r in refs:
        assert r.dtype == np.float32 and r.shape == (3, case.crop, case.crop)
        r.setflags(write=False)
    return tuple(refs)


def _ksize(n_in, n_out, kind):
    """Pillow's precompute_coeffs: ksize = ceil(support * max(in / out, 1)) * 2 + 1."""
    support = 2.0 if kind == "bicubic" else 1.0
    return int(math.ceil(support * max(n_in / n_out, 1.0))) * 2 + 1


def _offsets(case):
    """torchvision center_crop offsets, rounded half to even."""
    nh, nw = T.resize_size(*case.hw, case.resize)
    return int(round((nh - case.crop) / 2.0)), int(round((nw - case.crop) / 2.0))


# ---------------------------------------------------------------- premises (no GPU)

@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_premise_geometry(case):
    h, w = case.hw
    nh, nw = T.resize_size(h, w, case.resize)
    assert (nh, nw) == case.nhw
    assert ((nh - case.crop) / 2.0, (nw - case.crop) / 2.0) == case.offs
    assert case.crop <= nh and case.crop <= nw  # torchvision would pad otherwise
    assert (_ksize(w, nw, case.kind), _ksize(h, nh, case.kind)) == case.taps
    # the oracle's tables have the same width
    assert T._coeffs(w, nw, case.kind)[1].shape[1] == case.taps[0]
    assert T._coeffs(h, nh, case.kind)[1].shape[1] == case.taps[1]
    t = _tf(case)
    mean, std = _stats(case)
    assert (t.resize, t.crop, t.interpolation, t.preprocess) == (case.resize, case.crop, case.kind, True)
    assert np.array_equal(t.mean, np.asarray(mean, np.float32))
    assert np.array_equal(t.std, np.asarray(std, np.float32))
    imgs = _images(case.name)
    assert len(imgs) == (4 if case in SAT_CASES else 2)
    assert all(im.shape == (h, w, 3) and im.dtype == np.uint8 for im in imgs)
    assert not np.array_equal(imgs[0], imgs[1])
    assert max(h, w) <= 500


def test_premise_what_the_cases_reach():
    """The edges named in the docstring, read off the case tables."""
    blocks = lambda c: (c.crop + 255) // 256  # noqa: E731  column blocks of k_tf_horiz / k_tf_vert
    live = lambda c: c.crop - 256 * (blocks(c) - 1)  # noqa: E731  live threads of the last block
    b = BY_NAME
    assert (blocks(b["crop513-three-blocks"]), live(b["crop513-three-blocks"])) == (3, 1)
    assert (blocks(b["crop257-one-live-column"]), live(b["crop257-one-live-column"])) == (2, 1)
    assert (blocks(b["crop256-full-block"]), live(b["crop256-full-block"])) == (1, 256)
    assert blocks(b["dino518"]) == 3 and all(blocks(c) == 2 for c in BLOCK_CASES[:5])
    # k_tf_coeffs: 128 threads per block over 2 * crop indices, beyond the 4 blocks of crop 224
    assert all((2 * c.crop + 127) // 128 > 4 for c in BLOCK_CASES if c.crop > 256)
    assert (2 * 518 + 127) // 128 == 9
    # .5 offsets that round up under half-to-even and down under truncation, and ones that round down
    assert _offsets(b["crop513-three-blocks"]) == (44, 164)
    assert _offsets(b["left-59.5-up"]) == (16, 60) and _offsets(b["top-59.5-up"]) == (60, 16)
    assert _offsets(b["crop1"]) == (128, 178) and _offsets(b["crop255"]) == (0, 52)
    assert _offsets(b["taps63-124x248-bicubic-crop5"]) == (2, 6)
    assert _offsets(b["sat-clip-300x420"]) == (0, 44) and _offsets(b["sat-clip-64x90"]) == (0, 46)
    assert _offsets(b["dino518"]) == (0, 104)
    # an axis whose size already equals the target: Pillow skips the pass, the kernel filters
    for name in ("clip336-336x400-identity-rows", "clip-224x300-identity-rows"):
        assert b[name].hw[0] == b[name].nhw[0] and b[name].kind == "bicubic"
    assert b["left-59.5-up"].hw == b["left-59.5-up"].nhw
    assert b["1x7"].nhw == (256, 1792) and _offsets(b["1x7"]) == (16, 784)
    assert b["clip336-64x90-upscale"].nhw[0] / 64 == 5.25
    # the tap limit of `double w[64]`: 63 accepted on both axes, 65 refused on either
    assert all(c.taps == (63, 63) for c in TAP_OK_CASES)
    assert [c.taps for c in TAP_REFUSED_CASES] == [(65, 65), (65, 65), (65, 63)]


def _dense(n_in, n_out, kind, lo, n):
    """(n, n_in) matrix of the fixed-point coefficients of output indices [lo, lo + n)."""
    bounds, kk = T._coeffs(n_in, n_out, kind)
    K = np.zeros((n, n_in), np.float64)  # |sums| < 2^31: exact in float64
    for o in range(n):
        s, m = bounds[lo + o]
        K[o, s:s + m] = kk[lo + o, :m]
    return K


def _unclipped(img, resize, crop, kind):
    """(horizontal, vertical) pass values (2^21 + sum) >> 22 before clip8, for the crop's columns
    over the rows its rows read, and for the crop itself; and the clipped crop."""
    H, W, _ = img.shape
    nh, nw = T.resize_size(H, W, resize)
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    Kh, Kv = _dense(W, nw, kind, left, crop), _dense(H, nh, kind, top, crop)
    half = 1 << (T.PREC - 1)
    hs = (np.einsum("hwc,xw->hxc", img.astype(np.float64), Kh).astype(np.int64) + half) >> T.PREC
    rows = np.flatnonzero(np.any(Kv != 0, axis=0))
    tmp = np.clip(hs, 0, 255)
    vs = (np.einsum("hxc,yh->yxc", tmp.astype(np.float64), Kv).astype(np.int64) + half) >> T.PREC
    return hs[rows], vs, np.clip(vs, 0, 255).astype(np.uint8), (top, left)


@pytest.mark.parametrize("case", SAT_CASES, ids=_ids(SAT_CASES))
def test_premise_saturation(case):
    for pat, img in zip(PATTERNS, _images(case.name)):
        hs, vs, clipped, (top, left) = _unclipped(img, case.resize, case.crop, case.kind)
        # the sums are the ones Pillow's two passes form: clipped, they give its crop
        nh, nw = case.nhw
        full = T.resample(img, nw, nh, case.kind)
        assert np.array_equal(clipped, full[top:top + case.crop, left:left + case.crop]), pat
        if case.kind == "bilinear":
            assert 0 <= hs.min() and hs.max() <= 255 and 0 <= vs.min() and vs.max() <= 255, pat
        elif pat == "checker2":
            assert hs.min() < 0 and hs.max() > 255, (hs.min(), hs.max())
            assert vs.min() < 0 and vs.max() > 255, (vs.min(), vs.max())


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_premise_oracle_matches_pillow(case):
    mean, std = _stats(case)
    for img, ref in zip(_images(case.name), _refs(case.name)):
        got = T.transform(img, case.resize, case.crop, mean, std, case.kind)
        assert got.dtype == np.float32 and np.array_equal(got, ref)


# ---------------------------------------------------------------- DeviceTransform (GPU)

def _check(case):
    imgs, refs = _images(case.name), _refs(case.name)
    got = _tf(case).batch(list(imgs)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (len(imgs), 3, case.crop, case.crop)
    for i, ref in enumerate(refs):
        bad = np.argwhere(got[i] != ref)
        assert np.array_equal(got[i], ref), (case.name, i, len(bad), bad[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("case", BLOCK_CASES, ids=_ids(BLOCK_CASES))
def test_crops_beyond_one_column_block(dev, case):
    _check(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLACE_CASES, ids=_ids(PLACE_CASES))
def test_crop_placement_and_degenerate_geometry(dev, case):
    _check(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SAT_CASES, ids=_ids(SAT_CASES))
def test_saturating_images(dev, case):
    _check(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TAP_OK_CASES, ids=_ids(TAP_OK_CASES))
def test_tap_limit_accepted(dev, case):
    _check(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TAP_REFUSED_CASES, ids=_ids(TAP_REFUSED_CASES))
def test_tap_limit_refused(dev, case):
    from visreps_amd._lib import VisrepsHipError

    with pytest.raises(VisrepsHipError, match="downscale factor too large"):
        _tf(case).batch(list(_images(case.name)))
    _check(TAP_OK_CASES[0])  # the refusal leaves the library usable


@pytest.mark.gpu
def test_totensor_only(dev):
    """get_transform(preprocess=False): transforms.ToTensor(), one fp32 division per value."""
    from visreps_amd.dataloaders.obj_cls import get_transform

    ramp = np.arange(256, dtype=np.int64).reshape(16, 16)
    imgs = [np.stack([(ramp + 85 * c) % 256 for c in range(3)], axis=2).astype(np.uint8), _img(16, 16, 77)]
    assert all(np.unique(imgs[0][..., c]).size == 256 for c in range(3))  # every quotient v / 255
    t = get_transform(preprocess=False)
    got = t.batch(imgs).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (2, 3, 16, 16)
    for i, im in enumerate(imgs):
        ref = np.transpose(im, (2, 0, 1)).astype(np.float32) / np.float32(255)
        assert np.array_equal(got[i], ref), np.argwhere(got[i] != ref)[:4].tolist()
    assert np.array_equal(t(imgs[1]).cpu().numpy(), got[1])
    with pytest.raises(ValueError):
        t.batch([imgs[0], _img(16, 17, 78)])


# ---------------------------------------------------------------- the C entry point (GPU)

FILL = 0xA5
PAD = 1 << 16  # guard bytes on each side of a region


def _filter_id(kind):
    return {"bilinear": 0, "bicubic": 1}[kind]


def _call(dev, src, B, hw, resize, crop, filt, mean, std, out_ptr, ws_ptr, ws_bytes):
    """vr_transform_u8 on torch's current stream; (status, vr_last_error text)."""
    import torch

    from visreps_amd._lib import lib, stream_of

    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    with torch.cuda.device(dev):
        rc = lib().vr_transform_u8(src.data_ptr(), B, hw[0], hw[1], resize, crop, filt, mean.ctypes.data,
                                   std.ctypes.data, out_ptr, ws_ptr, ws_bytes, stream_of(dev))
    torch.cuda.synchronize(dev)
    return rc, lib().vr_last_error().decode(errors="replace")


def _src(imgs, dev):
    """(B, H, W, 3) uint8 on the device, densely packed."""
    import torch

    src = torch.from_numpy(np.stack(imgs)).to(dev)
    assert src.is_contiguous() and src.dtype == torch.uint8
    return src


def _guarded(nbytes, dev):
    """A FILL-filled buffer with `nbytes` at offset PAD and PAD guard bytes after them."""
    import torch

    buf = torch.full((PAD + nbytes + PAD,), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:PAD] == FILL).all()) and bool((buf[PAD + nbytes:] == FILL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", GUARD_CASES, ids=_ids(GUARD_CASES))
def test_entry_writes_only_out_and_exact_workspace(dev, case):
    import torch

    from visreps_amd._lib import lib

    imgs, refs = _images(case.name), _refs(case.name)
    B, crop, filt = len(imgs), case.crop, _filter_id(case.kind)
    mean, std = _stats(case)
    src = _src(imgs, dev)
    need = lib().vr_transform_workspace(B, *case.hw, case.resize, crop, filt)
    assert need > 0 and need % 256 == 0
    out_bytes = B * 3 * crop * crop * 4
    runs = []
    for _ in range(2):
        obuf, wbuf = _guarded(out_bytes, dev), _guarded(need, dev)
        rc, err = _call(dev, src, B, case.hw, case.resize, crop, filt, mean, std, obuf.data_ptr() + PAD,
                        wbuf.data_ptr() + PAD, need)
        assert rc == 0, err
        assert _guards_intact(obuf, out_bytes), "wrote outside out"
        assert _guards_intact(wbuf, need), "wrote outside the workspace"
        runs.append(obuf[PAD:PAD + out_bytes].cpu().numpy().view(np.float32).reshape(B, 3, crop, crop))
    assert np.array_equal(runs[0], runs[1])  # repeatable
    assert np.array_equal(runs[0], _tf(case).batch(list(imgs)).cpu().numpy())
    for i, ref in enumerate(refs):
        assert np.array_equal(runs[0][i], ref)


@pytest.mark.gpu
def test_entry_refusals_leave_out_unwritten(dev):
    import torch

    from visreps_amd._lib import lib

    case = BY_NAME["crop257-one-live-column"]
    imgs = _images(case.name)
    B, crop = len(imgs), case.crop
    mean, std = _stats(case)
    src = _src(imgs, dev)
    need = lib().vr_transform_workspace(B, *case.hw, case.resize, crop, 0)
    ws = torch.empty(need + (1 << 20), dtype=torch.uint8, device=dev)
    # crop 257 of a 256-high resize still fits this out
    out = torch.full((B * 3 * crop * crop * 4,), FILL, dtype=torch.uint8, device=dev)

    def refused(text, resize=case.resize, filt=0, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel()):
        rc, err = _call(dev, src, B, case.hw, resize, crop, filt, mean, std, out.data_ptr(), ws_ptr, ws_bytes)
        assert rc != 0 and text in err, (rc, err)
        assert bool((out == FILL).all()), text

    refused("filter 2", filt=2)
    assert T.resize_size(*case.hw, 256)[0] < crop
    refused("torchvision pads", resize=256)
    refused(f"workspace {need - 1} < {need}", ws_bytes=need - 1)
    refused("null pointer", ws_ptr=None, ws_bytes=need)
    # B = 0 is no error and no launch
    rc, err = _call(dev, src, 0, case.hw, case.resize, crop, 0, mean, std, out.data_ptr(), ws.data_ptr(),
                    ws.numel())
    assert rc == 0, err
    assert bool((out == FILL).all())
    # and the same arguments, unrefused, run
    rc, err = _call(dev, src, B, case.hw, case.resize, crop, 0, mean, std, out.data_ptr(), ws.data_ptr(), need)
    assert rc == 0, err
    got = out.cpu().numpy().view(np.float32).reshape(B, 3, crop, crop)
    for i, ref in enumerate(_refs(case.name)):
        assert np.array_equal(got[i], ref)


@pytest.mark.gpu
def test_entry_workspace_sizes(dev):
    from visreps_amd._lib import lib

    ws = lib().vr_transform_workspace
    good = [2, 300, 420, 256, 224]
    assert ws(*good, 0) > 0 and ws(*good, 1) > 0
    for i in range(len(good)):
        for bad in (0, -1):
            args = list(good)
            args[i] = bad
            assert ws(*args, 0) == 0, args
    assert ws(*good, 2) == 0 and ws(*good, -1) == 0
