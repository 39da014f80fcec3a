"""Writes tests/golden/image_items.npz: small random uint8 RGB images and what Pillow's own
`Image.fromarray(img).resize((OW, OH), Image.BILINEAR)` makes of them, for a few of the shapes of
tests/image_items_ref.py (and 75 x 75 -> 4 x 4, the 39 taps of 300 -> 16 on a small input).

    python tests/golden/gen_image_items.py

Keys: '<H>x<W>_<OH>x<OW>/img' u8[H, W, 3], '.../out' u8[OH, OW, 3]; 'meta/pillow' the Pillow version."""
import os

import numpy as np
from PIL import Image
import PIL

CASES = [(7, 5, 3, 4), (5, 9, 8, 16), (9, 224, 5, 128), (64, 64, 128, 128), (137, 137, 128, 128), (75, 75, 4, 4)]


def main():
    rng = np.random.default_rng(20261019)
    out = {"meta/pillow": np.array(PIL.__version__)}
    for H, W, OH, OW in CASES:
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        if (H, W) == (7, 5):
            img[0, 0], img[-1, -1] = 255, 0                   # the extremes at the clipped borders
        res = np.asarray(Image.fromarray(img, "RGB").resize((OW, OH), Image.BILINEAR))
        name = "%dx%d_%dx%d" % (H, W, OH, OW)
        out[name + "/img"], out[name + "/out"] = img, res
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_items.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
