"""k_present (csrc/rtx_present.h) on images no render produces, at frame sizes down to one pixel.

The kernel is specified bit for bit against the oracle's orc_present, but tests/test_present.py feeds it rendered frames only: smooth images
at a few sizes, none smaller than a 16 x 16 launch block.  rtx_present reads whatever framebuffer is bound, so any image can be presented
without rendering it.  Here, per frame size, one context on the cube scene gets a pair of torch tensors bound as its framebuffer, the packed
one filled with
    noise          seeded, over all 24 bits
    checkerboard   one-pixel squares of 0xffffff and 0: all four diagonal taps carry the centre's colour, so the filter must leave the image
                   alone although every neighbour differs; where a side is odd the wrap-around seam breaks the pattern and it must not
    black or white random: flat runs broken by full-contrast edges in every direction
    one channel    random pixels with a single channel at 255: edges whose luma steps are 0.299, 0.587 and 0.114
and present(fxaa) must equal orc.present(image, fxaa), identity and FXAA.  Sizes: one pixel, single rows and columns (every tap wraps to the
same row or column under GL_REPEAT), below, at and above one launch block, odd, and not square (the shader scales the vertical tap offsets
by 1 / width, which only a frame that is not square shows).  Afterwards the binding is lifted, the context renders, and what it presents is
its own frame again."""
import numpy as np
import pytest

import util

SIZES = [(1, 1), (1, 2), (2, 1), (1, 17), (17, 1), (3, 5), (15, 17), (16, 16), (33, 31), (47, 129)]      # (height, width)
KINDS = ("noise", "checkerboard", "black or white", "one channel")


def image(kind, h, w):
    rng = np.random.default_rng([KINDS.index(kind), h, w])
    if kind == "noise":
        return rng.integers(0, 1 << 24, (h, w), dtype=np.uint32)
    if kind == "checkerboard":
        return np.where((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0, 0xffffff, 0).astype(np.uint32)
    if kind == "black or white":
        return np.where(rng.integers(0, 2, (h, w)) == 1, 0xffffff, 0).astype(np.uint32)
    return (np.uint32(255) << (rng.integers(0, 3, (h, w)) * 8).astype(np.uint32)).astype(np.uint32)


def sized_scene(h, w):
    sc, _ = util.load_golden("cube")
    sc.config = sc.config.copy()
    sc.config["width"] = w; sc.config["height"] = h
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_present_of_bound_images_equals_the_oracle(h, w):
    import orc
    import torch
    from pyrtx import api
    sc = sized_scene(h, w)
    assert (sc.height, sc.width) == (h, w)
    r = api.Renderer(sc)
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    packed = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    r.bind_framebuffer(rgb.data_ptr(), packed.data_ptr())
    for kind in KINDS:
        img = image(kind, h, w)
        assert img.shape == (h, w) and img.dtype == np.uint32 and int(img.max()) < 1 << 24
        packed.copy_(torch.from_numpy(img.astype(np.int32)))
        torch.cuda.synchronize()
        for fxaa in (False, True):
            got, want = r.present(fxaa), orc.present(img, fxaa)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (f"{h} x {w} {kind} fxaa {fxaa}: {len(bad)} pixels differ, first (y, x) {bad[:5].tolist()}: "
                                   f"got {[hex(v) for v in got[got != want][:5]]} want {[hex(v) for v in want[got != want][:5]]}")
        assert np.array_equal(packed.cpu().numpy().view(np.uint32), img), kind          # presenting reads the frame only
    # the binding lifted: the context renders into and presents its own frame again, not the last image bound
    r.bind_framebuffer(None, None)
    out = r.render()
    ref = orc.OracleScene(sc).render(threads=2)
    assert np.array_equal(out["packed"], ref["packed"]) and util.bit_exact(out["rgb"], ref["rgb"])
    for fxaa in (False, True):
        assert np.array_equal(r.present(fxaa), orc.present(ref["packed"], fxaa)), fxaa
    assert np.array_equal(packed.cpu().numpy().view(np.uint32), image(KINDS[-1], h, w))   # and the tensors that were bound are left alone
    r.close()


def test_the_images_are_hostile():
    """No GPU: what the images are for, on the oracle.  In a random image the four diagonal lumas differ at almost every pixel, so the blur
    direction is not zero and the taps, up to 8 texels away, land on other texels: FXAA changes at least a tenth of the pixels of every
    random two-dimensional case.  The even checkerboard is a fixed point, the odd ones are not."""
    import orc
    changed = lambda img: float((orc.present(img, True) != orc.present(img, False)).mean())
    for h, w in SIZES:
        if min(h, w) < 3:
            continue
        for kind in ("noise", "black or white", "one channel"):
            assert changed(image(kind, h, w)) > 0.1, (h, w, kind)
        assert (changed(image("checkerboard", h, w)) == 0) == (h % 2 == 0 and w % 2 == 0), (h, w)
