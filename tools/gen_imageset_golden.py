"""Writes tests/golden/imagesets/pil_resize.npz: source images and what PIL's own `Image.resize(..., BILINEAR)` makes of them
(mode L, the path torchvision's Resize takes on the PIL images of the MNIST family), for tests/test_21_imagesets_gpu.py - PIL
need not be installed where the GPU tests run.  Needs Pillow.

    python tools/gen_imageset_golden.py
"""
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'imagesets', 'pil_resize.npz')


def resize(images, Hr, Wr, turn=False):
    out = []
    for a in images:
        img = Image.fromarray(a, mode='L')
        if turn:
            img = img.rotate(90, expand=True)
        out.append(np.asarray(img.resize((Wr, Hr), Image.BILINEAR)))
    return np.stack(out)


def main():
    rng = np.random.default_rng(2024)
    s28 = rng.integers(0, 256, (6, 28, 28), dtype=np.uint8)
    s28[1] = 255
    s28[2] = (rng.random((28, 28)) < 0.5) * np.uint8(255)
    s28[3, :, :14] = 0                                         # a hard edge
    s75 = rng.integers(0, 256, (3, 7, 5), dtype=np.uint8)
    s32 = rng.integers(0, 256, (3, 32, 32), dtype=np.uint8)
    rec = {'src_28_32': s28, 'out_28_32': resize(s28, 32, 32),
           'src_7x5_9x8': s75, 'out_7x5_9x8': resize(s75, 9, 8),
           'src_32_28': s32, 'out_32_28': resize(s32, 28, 28),
           'src_turn_7x5_8x9': s75, 'out_turn_7x5_8x9': resize(s75, 8, 9, turn=True)}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **rec)
    print('wrote', OUT, {k: v.shape for k, v in rec.items()})


if __name__ == '__main__':
    main()
