"""The tile records of a sketch plane (include/sketchedit_hip.h, se_sketch_tiles_u8) restated in numpy: the
oracle of the kernel (tests/test_gpu_regions.py) and the tiles call of the host tests' stand-in backend
(tests/test_regions_host.py)."""
import numpy as np


def sketch_tiles(sketch, tile):
    """sketch (Hi,Wi) uint8 -> (ceil(Hi / tile), ceil(Wi / tile), 5) int32 of [count, y0, x0, y1, x1]: the pixels > 0 of every
    tile x tile square and their tight half-open box in frame coordinates; five zeros for an empty square."""
    sketch = np.asarray(sketch)
    Hi, Wi = sketch.shape
    nty, ntx = -(-Hi // tile), -(-Wi // tile)
    out = np.zeros((nty, ntx, 5), np.int32)
    for ty in range(nty):
        for tx in range(ntx):
            ys, xs = np.nonzero(sketch[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile] > 0)
            if ys.size:
                out[ty, tx] = (ys.size, ty * tile + ys.min(), tx * tile + xs.min(), ty * tile + ys.max() + 1, tx * tile + xs.max() + 1)
    return out
