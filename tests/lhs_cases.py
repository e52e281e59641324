"""Shared cases of the stratified-sampler tests (test_lhs_replay.py, test_gpu_lhs.py,
test_gpu_first_ball_regimes.py): the walk counts of the full-solve sweep, the point
indices whose shuffle hits PCG32's rejection threshold, and a pure-Python PCG32 /
stratified sampler written from the oracle's definitions (oracle/wos_oracle.c pcg_seed,
pcg_next, pcg_bounded, oracle_seed32, gen_stratified; sampling.h:435-457)."""
import numpy as np

KEY = 0x5EED0001

# full solves against the oracle (test_gpu_first_ball_regimes.py): (dim, nWalks, antithetic)
# (192 / 194 in 2D and 384 .. 514 are there for the plan coverage check of test_lhs_cpu.py: the
# LDS shuffle's third / fourth chunk and the pair loop's fourth and fifth pass)
SWEEP_2D = [1, 2, 3, 6, 32, 34, 42, 44, 64, 66, 126, 128, 130, 192, 194, 256, 258, 384, 386, 512, 514, 600]
SWEEP_3D = [2, 8, 32, 34, 42, 44, 64, 66, 128, 130, 192, 194, 256, 258, 384, 386, 512, 514]
SWEEP_NO_ANTI = [(2, 5), (2, 128), (2, 129), (3, 33), (3, 65)]


def sweep_cases():
    return ([(2, nw, True) for nw in SWEEP_2D] + [(3, nw, True) for nw in SWEEP_3D] +
            [(dim, nw, False) for dim, nw in SWEEP_NO_ANTI])


def n_pairs_of(n_walks, anti):
    """wos_capi_solve.cpp dev_params: walks per antithetic iteration set."""
    return max(1, n_walks // 2) if anti else n_walks


# (nstrat, dim - 1) -> point indices whose shuffle draws reject, key KEY, tag-0 stream
REPLAY = {
    (128, 1): [1348635, 1801287, 1964175],
    (64, 2): [3569100, 3925263, 4995051],
    (256, 1): [14017, 812531, 1149871],
    (200, 2): [211192, 828713, 869192],
    (600, 1): [73031, 127857, 184932],
}

M64 = (1 << 64) - 1
PCG_MULT = 0x5851F42D4C957F2D


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def seed32(key, idx, pair, tag):
    h = mix64(key ^ mix64((idx * 0x9E3779B97F4A7C15 + pair * 0xD1B54A32D192ED03 + tag * 0x8CB92BA72F3D8DD7 +
                           0x632BE59BD9B4E019) & M64))
    return h >> 32


class Pcg32:
    def __init__(self, initstate, initseq=1):
        self.state, self.inc = 0, ((initseq << 1) | 1) & M64
        self.next()
        self.state = (self.state + initstate) & M64
        self.next()

    def next(self):
        old = self.state
        self.state = (old * PCG_MULT + self.inc) & M64
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF

    def uniform(self):
        return np.array([(self.next() >> 9) | 0x3F800000], np.uint32).view(np.float32)[0] - np.float32(1.0)


def lhs_python(seed, n, dims):
    """gen_stratified on Pcg32(seed): (samples float32 [n * dims], rejected draws)."""
    g = Pcg32(seed)
    ome = np.float32(1.0) - np.finfo(np.float32).eps
    inv = np.float32(1.0) / np.float32(n)
    s = np.zeros(n * dims, np.float32)
    for i in range(n):
        for j in range(dims):
            s[dims * i + j] = min((np.float32(i) + g.uniform()) * inv, ome)
    rejected = 0
    for i in range(dims):
        for j in range(n):
            bound = n - j
            th = (1 << 32) % bound
            r = g.next()
            while r < th:  # pcg_bounded: redraw below 2^32 mod bound
                rejected += 1
                r = g.next()
            other = j + r % bound
            s[dims * j + i], s[dims * other + i] = s[dims * other + i], s[dims * j + i]
    return s, rejected
