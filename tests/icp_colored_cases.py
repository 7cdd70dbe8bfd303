"""What the Colored-ICP tests with and without a GPU share: the robust-kernel cases of the scene and the restatement's
colour gradients of the scene's target, computed once per (seed, max_nn) and left unchanged."""
import functools

import icp_colored_reference as RC

# kernel parameters at the scale of the scene's residuals (geometric ~ 1e-3, photometric ~ 4e-3), so every kernel bites
KERNEL_CASES = [("l2", 1.0), ("huber", 0.002), ("cauchy", 0.002), ("gm", 0.002), ("tukey", 0.01)]


@functools.lru_cache(maxsize=None)
def scene(seed=0):
    return RC.scene(seed)


@functools.lru_cache(maxsize=None)
def scene_gradients(seed=0, max_nn=30):
    s = scene(seed)
    g = RC.color_gradients(s["target"], s["target_normals"], s["target_colors"], 2 * s["r"], max_nn)
    g.setflags(write=False)
    return g
