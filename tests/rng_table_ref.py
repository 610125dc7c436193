"""The table of scatter draws restated in plain Python (option
rng_table): for the path whose first seed is s0 = y * width + x, the seed takes
the primary ray's two draws, and then each scatter takes three discarded draws
and tries of three draws, p = 2 * r - 1 in binary32, until dot(p, p) < 1.
Entry k holds the accepted point and the seed after it.

Integers are Python ints masked to 32 bits; floats are numpy.float32 scalars,
so every operation rounds to binary32 as the kernels' do.  tests/
test_gpu_rng_table.py pins pcg to oracle/shader_np.py's."""
import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
MAX_REJECT_TRIPLES = 1 << 16


def pcg(v: int) -> int:
    s = (v * 747796405 + 2891336453) & M32
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & M32
    return (w >> 22) ^ w


def draw(seed: int):
    """(seed', float(seed') / 2^32 in binary32): uint -> float rounds to nearest even."""
    seed = pcg(seed)
    return seed, F(seed) / F(4294967296.0)


def in_sphere(seed: int):
    """(seed', (x, y, z)) of one randomVec3InUnitSphere call."""
    seed = pcg(pcg(pcg(seed)))
    for _ in range(MAX_REJECT_TRIPLES):
        seed, a = draw(seed)
        seed, b = draw(seed)
        seed, c = draw(seed)
        x, y, z = a * F(2.0) - F(1.0), b * F(2.0) - F(1.0), c * F(2.0) - F(1.0)
        if (x * x + y * y) + z * z < F(1.0):
            return seed, (x, y, z)
    return seed, (F(0.0), F(0.0), F(0.0))


def table(width: int, height: int, k: int) -> np.ndarray:
    """uint32 [k, height, width, 4]: the bits of p.x, p.y, p.z and the seed."""
    out = np.zeros((k, height, width, 4), np.uint32)
    for s0 in range(width * height):
        seed = pcg(pcg(s0))                      # the primary ray's jitter pair
        for j in range(k):
            seed, p = in_sphere(seed)
            out[j, s0 // width, s0 % width, :3] = np.array(p, F).view(np.uint32)
            out[j, s0 // width, s0 % width, 3] = seed
    return out
