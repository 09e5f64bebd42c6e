"""A small folder of pictures for the prepare_data tests, and Pillow's own resize + centre crop of a file."""
import os

import numpy as np

from stylerenderer_amd.op import resample


def make_folder(root, seed=0):
    """Pictures of several shapes in nested folders, one file that is no picture and one truncated JPEG.
    Returns the readable paths in sorted order."""
    from PIL import Image

    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "b", "deep"))
    os.makedirs(os.path.join(root, "a"))
    shapes = {"a/one.png": (40, 52), "a/two.PNG": (61, 37), "b/three.jpg": (48, 48), "b/deep/four.bmp": (33, 70),
              "five.png": (40, 52), "b/deep/six.png": (40, 52)}
    for rel, (h, w) in shapes.items():
        # smooth content plus noise: JPEG sources decode to something resampling filters tell apart
        y, x = np.mgrid[0:h, 0:w]
        img = np.stack([(x * 5 + y * 3) % 256, (x * y) % 256, rs.randint(0, 256, (h, w))], 2).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, rel), **({"quality": 95} if rel.endswith("jpg") else {}))
    with open(os.path.join(root, "notes.txt"), "w") as f:
        f.write("not a picture")
    whole = open(os.path.join(root, "b", "three.jpg"), "rb").read()
    with open(os.path.join(root, "a", "broken.jpg"), "wb") as f:
        f.write(whole[:len(whole) // 3])
    return sorted(os.path.join(root, rel) for rel in shapes)


def pillow_levels(path, size, flt):
    from PIL import Image

    im = Image.open(path).convert("RGB")
    w, h = im.size
    (oh, ow), (top, left, _, _) = resample.center_crop_geometry(h, w, size)
    return np.asarray(im.resize((ow, oh), flt).crop((left, top, left + size, top + size)))
