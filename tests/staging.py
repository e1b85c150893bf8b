"""Worlds at the limits of the step kernels' LDS staging, their start states, and the oracle's run through them.

step_local_kernel's prologue copies the shared geometry into LDS: the path (up to 24 KB = 614 way points of five doubles, one
double per stager and a strided loop for what is left) and the lethal bitmap (up to kLocalMapWords = 4 096 words, 6 / 11 / 22
words per stager in slices of 768 / 384 / 192).  The worlds here sit on both sides of those limits and put their lethal cells
and the envs' way points where only the late slices and the loop's trips reach:
  limit_map    a walled map of exactly `words` bitmap words whose only other lethal cells are speckles in rows that lie wholly
               at word 2 304 (the start of the fourth slice of 768) or later
  limit_path   exactly n_way way points wound through a region of a map
  dense_path   way points 0.4 mm apart: a block of 64 envs has far more than kScanItems = 1 024 of them in its windows
  start_batch  start states in the style of util.random_batch: scattered along the whole path, a group before the last five
               way points, a third aimed at speckles
  run_oracle   the oracle's steps through a case; path_conditions, map_conditions and scan_candidates say what those steps
               show about the inputs

Plain module (no fixtures), numpy and the oracle only: imported by test_staging_host.py and test_gpu_step_staging.py.  Nothing
here imports the GPU package at module level.
"""
import os

import numpy as np

import footprints as F
from util import GOLDEN

# ---- constants restated from csrc/bcp_step_layout.h (test_staging_host.py compares them with what a compiler saw there) ----
LOCAL_MAP_WORDS = 4096       # kLocalMapWords
PATH_LDS_BYTES = 24 * 1024   # kPathLdsBytes: a shared path of at most this many bytes is staged
WAY_POINT_BYTES = 5 * 8      # x, y, heading, cos, sin
MAX_STAGED_WAY_POINTS = PATH_LDS_BYTES // WAY_POINT_BYTES   # 614
SCAN_ITEMS = 1024            # kScanItems
PAIR_STAGE_DOUBLES = 512     # step_fast_pair_kernel: path doubles staged from registers (4 per thread of 128)
STAGERS = 768                # staging threads of a 16-wave workgroup
FOURTH_SLICE = 3 * STAGERS   # 2 304: first word beyond the third slice of the bitmap staging
assert MAX_STAGED_WAY_POINTS == 614 and FOURTH_SLICE == 2304

RES = 0.05
SP, AP, TIMEOUT = 0.2, np.pi / 8, 60
N, STEPS = 256 + 37, 24
TAIL = 50                    # envs started just before the last five way points
LIMIT_SHAPES = {4095: (273, 470), 4096: (256, 500), 4097: (241, 530), 2305: (461, 150)}
PATH_LENGTHS = (38, 39, 76, 77, 102, 103, 153, 154, 614, 615)
WIDE_SCALE, WIDE_RES = 1.7, 0.03


def bitmap_words(shape):
    return shape[0] * ((shape[1] + 31) // 32)


def word_of(shape):
    """word index of every cell of a map of `shape` in its lethal bitmap -> int [rows, cols]"""
    rows, cols = shape
    wpr = (cols + 31) // 32
    return np.arange(rows)[:, None] * wpr + np.arange(cols)[None, :] // 32


def _extent(verts):
    """(front reach along +x, largest |y|, radius) of a footprint"""
    v = np.asarray(verts, dtype=np.float64)
    return float(v[:, 0].max()), float(np.abs(v[:, 1]).max()), F.radius(v)


def _region_of_rows(origin, res, shape, row0, row1, verts):
    """the rectangle in which paths run: rows row0 .. row1 of the map, all columns, less a margin in which a robot on the path
    clears the walls sideways -> (x0, x1, y0, y1) in metres"""
    _, half_w, r = _extent(verts)
    return (origin[0] + r + 0.3, origin[0] + (shape[1] - 1) * res - r - 0.3,
            origin[1] + row0 * res + half_w + 0.35, origin[1] + row1 * res - half_w - 0.35)


def _start_pose(region):
    """where every path of a region begins: the middle of its left edge (limit_map keeps the speckles away from there)"""
    return region[0], 0.5 * (region[2] + region[3])


def limit_map(oracle, words, verts=F.TRICYCLE, res=RES, seed=0):
    """A walled map of LIMIT_SHAPES[words] whose bitmap has exactly `words` words; the columns are no multiple of 32, so the
    last word of every row is partial.  Apart from the wall the lethal cells are isolated speckles at speckle_world's density
    (0.7 / pixels of the footprint: about one under every second footprint), all of them in rows whose first word is at index
    2 304 or later, none near the first pose of the region's paths.
    In the 2 305-word map no row lies wholly at or beyond word 2 304 -- the only row that reaches it is the bottom wall -- so
    there the wall's own cells in word 2 304 (columns 128 .. 149 of the last row) are listed in the speckles' place, and the
    poses aimed at them come from above.
    -> dict(cm, origin, res, verts, words, region, speckles (rows, cols), speckle_words (the word index of every speckle), aim)"""
    rows, cols = LIMIT_SHAPES[words]
    assert bitmap_words((rows, cols)) == words and cols % 32
    rng = np.random.RandomState(100 + seed)
    wpr = (cols + 31) // 32
    first_row = -(-FOURTH_SLICE // wpr)         # rows r with r * wpr >= 2 304
    origin = np.array([-0.5 * cols * res, -0.5 * rows * res])
    cm = np.zeros((rows, cols), dtype=np.uint8)
    area = int(np.count_nonzero(oracle.pixel_footprint(0.3, verts, res)))
    aim = None
    if first_row <= rows - 2:
        region = _region_of_rows(origin, res, (rows, cols), first_row, rows - 1, verts)
        band = np.zeros((rows, cols), dtype=bool)
        band[first_row:rows - 1, 1:cols - 1] = rng.rand(rows - 1 - first_row, cols - 2) < 0.7 / area
        # isolated: no speckle next to another one
        sr, sc = np.nonzero(band)
        for r, c in zip(sr, sc):
            if band[r, c] and band[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2].sum() > 1:
                band[r, c] = False
        sx, sy = _start_pose(region)
        yy, xx = np.mgrid[0:rows, 0:cols]
        band[np.hypot(origin[0] + xx * res - sx, origin[1] + yy * res - sy) < F.radius(verts) + 0.4] = False
        cm[band] = 254
        sr, sc = np.nonzero(band)
    else:
        region = _region_of_rows(origin, res, (rows, cols), rows - 160, rows - 1, verts)
        sc = np.arange((FOURTH_SLICE - (rows - 1) * wpr) * 32, cols - 1)
        sr = np.full(len(sc), rows - 1)
        aim = (0.5 * np.pi, 0.5)                # headings towards the bottom wall (the last row is the largest y)
    cm[0, :] = cm[-1, :] = cm[:, 0] = cm[:, -1] = 254
    sw = word_of((rows, cols))[sr, sc]
    assert len(sw) >= 4 and (sw >= FOURTH_SLICE).all()
    return dict(cm=cm, origin=origin, res=res, verts=np.asarray(verts, dtype=np.float64), words=words, region=region,
                speckles=(sr, sc), speckle_words=sw, aim=aim)


def clear_goal(world, path):
    """the world without the speckles within a footprint's radius + 0.4 m of the path's last way point, as limit_map keeps them
    away from the first: episodes are to end at the goal, not on a speckle before it (walls stay)"""
    sr, sc = world["speckles"]
    x, y = world["origin"][0] + sc * world["res"], world["origin"][1] + sr * world["res"]
    rows, cols = world["cm"].shape
    gone = (np.hypot(x - path[-1, 0], y - path[-1, 1]) < F.radius(world["verts"]) + 0.4) & (sr > 0) & (sr < rows - 1) & (sc > 0) & (sc < cols - 1)
    cm = world["cm"].copy()
    cm[sr[gone], sc[gone]] = 0
    return dict(world, cm=cm, speckles=(sr[~gone], sc[~gone]), speckle_words=world["speckle_words"][~gone])


def golden_world():
    """the 183 x 183 map of the g8 mini trajectories (1 098 words, no wall around it): paths wind through its open upper part,
    the aimed poses go for the cells of its two walls"""
    g = np.load(os.path.join(GOLDEN, "g8_traj_mini_00.npz"))
    cm, origin, res = np.ascontiguousarray(g["costmap"]), np.asarray(g["origin"], dtype=np.float64), float(g["resolution"])
    sr, sc = np.nonzero(cm == 254)
    return dict(cm=cm, origin=origin, res=res, verts=F.TRICYCLE, words=bitmap_words(cm.shape), region=(-2.3, 2.3, 0.2, 2.5),
                speckles=(sr, sc), speckle_words=word_of(cm.shape)[sr, sc], aim=None)


def limit_path(n_way, world, spacing=0.1):
    """Exactly n_way way points, `spacing` apart along y = yc - A sin(2 pi (x - x0) / w) from the middle of the region's left
    edge (first away from the larger y, where limit_map's regions have their wall), headings along the tangent.  The period w
    is the widest of 3.2 .. 0.8 m at which the curve across the region is long enough; where even 0.8 m is not, the spacing
    shrinks instead.  Neighbouring way points are at most `spacing` < goal_spat_dist apart, legs of the curve at least 0.4 m."""
    x0, x1, y0, y1 = world["region"]
    yc, amp = 0.5 * (y0 + y1), 0.5 * (y1 - y0)
    assert spacing < SP and amp > 0.5 and x1 - x0 > 2.0
    t = np.linspace(0.0, x1 - x0, 40001)
    for w in (3.2, 2.4, 1.6, 1.2, 0.8):
        y = yc - amp * np.sin(2 * np.pi * t / w)
        arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(t), np.diff(y)))])
        if arc[-1] >= (n_way - 1) * spacing:
            break
    spacing = min(spacing, arc[-1] / (n_way - 1))
    at = np.interp(np.arange(n_way) * spacing, arc, t)
    path = np.stack([x0 + at, yc - amp * np.sin(2 * np.pi * at / w),
                     np.arctan2(-amp * 2 * np.pi / w * np.cos(2 * np.pi * at / w), 1.0)], axis=1)
    assert len(path) == n_way and np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1])).max() < SP
    assert np.hypot(*(path[-1, :2] - path[0, :2])) > 2 * SP       # the goal is away from the start
    return path


def dense_path(n_way, world, spacing=0.0004, radius=1.5):
    """n_way way points `spacing` apart on an arc of `radius` through the middle of the region: 0.24 m of path in all.
    A pose reaches every way point less than goal_spat_dist behind it, up to 500 of them, and target_idx then moves past
    the last one; from there on a robot at 0.25 m/s passes some 30 further way points per step.  (Laps wound over each other
    would add nothing after the first step: the target jumps to the last lap at once.  What keeps the candidate windows
    full step after step is the density along the direction of travel.)"""
    x0, x1, y0, y1 = world["region"]
    cx, cy = 0.5 * (x0 + x1), 0.5 * (y0 + y1) + radius
    phi = -0.5 * np.pi + np.arange(n_way) * spacing / radius
    return np.stack([cx + radius * np.cos(phi), cy + radius * np.sin(phi), phi + 0.5 * np.pi], axis=1)


def start_batch(rng, n, world, path, timeout=TIMEOUT, xy_sigma=0.15, th_sigma=0.3, tail=TAIL, zero_iter=False, v_min=0.0,
                early=0.0, target_back=0, wheel=True):
    """n start states in the style of util.random_batch: poses near random way points of the whole path, at a random iteration
    below `timeout` (the first eight one step before it; zero_iter: all at 0, for delay queues that must start empty).
      envs 8 .. 8 + tail   a few centimetres before one of the last five way points, heading and rolling along the path; the
                           second half of them before the last one, which is their target
      a third of the rest  aimed at a speckle: it lies straight ahead, under the footprint or just beyond its front
    The dense path's knobs: speeds from v_min up, a fraction `early` of the poses on the first 40 % of the path (they are still
    on it eight steps later), and targets `target_back` way points behind the pose's own (positions are scattered over
    hundreds of way points there: a target ahead of everything in reach would make the first step's window empty).
    wheel False: the wheel angle stays 0 (the diff-drive's state has none; the oracle's reset would clear it, the library's not).
    -> state [7, n], min_dist, target_idx, current_iter"""
    m = len(path)
    front, _, _ = _extent(world["verts"])
    idx = np.where(rng.rand(n) < early, rng.randint(0, max(2 * m // 5, 1), n), rng.randint(0, m, n))
    st = np.zeros((7, n))
    st[0] = path[idx, 0] + rng.normal(0, xy_sigma, n)
    st[1] = path[idx, 1] + rng.normal(0, xy_sigma, n)
    st[2] = path[idx, 2] + rng.normal(0, th_sigma, n)
    st[3] = rng.uniform(v_min, 0.5, n)
    st[4] = rng.uniform(-0.5, 0.5, n)
    st[6] = rng.uniform(-1.0, 1.0, n)
    tgt = np.clip(idx - target_back + rng.randint(-3, 4, n), 1, m - 1).astype(np.int32)
    # the tail of the path
    t = np.arange(8, 8 + tail)
    j = np.where(np.arange(tail) < tail // 2, m - 1 - np.arange(tail) % 5, m - 1)
    back, side = rng.uniform(0.0, 0.12, tail), rng.normal(0, 0.03, tail)
    back[tail // 2:] = rng.uniform(0.04, 0.12, tail - tail // 2)      # (not reached at once: -spat_dist / 9 = -0.022 along the heading)
    th = path[j, 2]
    st[0, t] = path[j, 0] - back * np.cos(th) - side * np.sin(th)
    st[1, t] = path[j, 1] - back * np.sin(th) + side * np.cos(th)
    st[2, t] = th + rng.normal(0, 0.08, tail)
    st[3, t] = rng.uniform(0.3, 0.5, tail)
    st[4, t] = rng.uniform(-0.1, 0.1, tail)
    st[6, t] = rng.uniform(-0.2, 0.2, tail)
    tgt[t] = j
    # the aimed third
    near = rng.rand(n) < 0.33
    near[:8 + tail] = False
    sr, sc = world["speckles"]
    pick = rng.randint(0, len(sr), n)
    ang = rng.uniform(-np.pi, np.pi, n) if world["aim"] is None else world["aim"][0] + rng.uniform(-1, 1, n) * world["aim"][1]
    dist, side = rng.uniform(0.2, 1.08, n) * front, rng.normal(0, 0.1, n)
    sx, sy = world["origin"][0] + sc[pick] * world["res"], world["origin"][1] + sr[pick] * world["res"]
    st[0] = np.where(near, sx - dist * np.cos(ang) - side * np.sin(ang), st[0])
    st[1] = np.where(near, sy - dist * np.sin(ang) + side * np.cos(ang), st[1])
    st[2] = np.where(near, ang, st[2])
    if not wheel:
        st[6] = 0.0
    md = np.hypot(path[tgt, 0] - st[0], path[tgt, 1] - st[1]) + rng.uniform(-0.01, 0.05, n)
    it = np.zeros(n, dtype=np.int32) if zero_iter else rng.randint(0, timeout, n).astype(np.int32)
    if not zero_iter:
        it[:8] = timeout - 1
    return st, md, tgt, it


# ---- the cases ------------------------------------------------------------------------------------------------------------------
class Case(object):
    """one world with its robot, start states and actions; built once per name (case()) and left alone"""

    def __init__(self, name, world, path, model="tricycle", noisy=True, delays=None, footprint_scale=1.0, timeout=TIMEOUT,
                 steps=STEPS, seed=0, v_scale=1.0, **start_knobs):
        if world["words"] in LIMIT_SHAPES:
            world = clear_goal(world, path)
        self.name, self.world, self.path = name, world, path
        self.cm, self.origin, self.res = world["cm"], world["origin"], world["res"]
        self.model, self.noisy, self.delays = model, noisy, dict(delays or {})
        self.footprint_scale, self.timeout, self.steps, self.v_scale = footprint_scale, timeout, steps, v_scale
        self.words, self.n_way = bitmap_words(self.cm.shape), len(path)
        self.staged_path = self.n_way <= MAX_STAGED_WAY_POINTS
        self.staged_map = self.words <= LOCAL_MAP_WORDS
        rng = np.random.RandomState(7 + seed)
        self.start = start_batch(rng, N, world, path, timeout, zero_iter=bool(self.delays), wheel=model == "tricycle",
                                 **start_knobs)
        lo, hi = (np.array([np.pi / 30, -np.pi / 2]), np.array([np.pi / 6, np.pi / 2]))   # BatchedPlanEnv.action_space
        rng = np.random.RandomState(11 + seed)
        if model == "tricycle":
            self.actions = [rng.uniform(lo, hi, (N, 2)).astype(np.float32) for _ in range(steps)]
        else:                                   # (the diff-drive takes v and w: test_gpu_step_variants' ranges)
            self.actions = [np.stack([rng.uniform(0.105, 0.524, N), rng.uniform(-np.pi / 2, np.pi / 2, N)], 1).astype(np.float32)
                            for _ in range(steps)]
        for a in self.actions:
            a[:, 0] *= v_scale
        self.host_z = [rng.standard_normal((N, 3)) for _ in range(steps)] if noisy else None
        for a in (self.cm, self.path) + tuple(self.start) + tuple(self.actions):
            a.setflags(write=False)

    def oracle_params(self, oracle):
        return oracle.make_params(self.model, noise=oracle.PLANENV_NOISE if self.noisy else None, spatial_precision=SP,
                                  angular_precision=AP, iteration_timeout=self.timeout, footprint_scale=self.footprint_scale,
                                  **self.delays)

    def env_params(self):
        from bc_gym_planning_env_amd import EnvParams
        robot = dict(tricycle='industrial_tricycle_v1', diffdrive='industrial_diffdrive_v1')[self.model]
        return EnvParams(goal_spat_dist=SP, goal_ang_dist=AP, resolution=self.res, refine_path=False, iteration_timeout=self.timeout,
                         robot_name=robot, **self.delays)

    def make_env(self, n_envs=N, seed=123):
        from bc_gym_planning_env_amd import BatchedPlanEnv, CostMap2D
        return BatchedPlanEnv(CostMap2D(self.cm.copy(), self.res, self.origin.copy()), self.path.copy(), self.env_params(), n_envs=n_envs,
                              noise_parameters='planenv' if self.noisy else None, footprint_scale=self.footprint_scale,
                              auto_reset=True, seed=seed)


_CASES = {}


def case(oracle, name):
    """The case of a name, built on first use:
      path-<n>      n way points on the golden map                           (n in PATH_LENGTHS)
      map-<words>   a 154-point path on limit_map(words)                     (words in LIMIT_SHAPES)
      max-delays    4 096 words, 614 way points, tricycle with all three delay queues (the largest LDS request)
      max-diffdrive 4 096 words, 614 way points, the 24-vertex diff-drive, no noise
      max-wide      4 096 words at 0.03, the tricycle scaled by 1.7 (the WIDE kernels), 154 way points
      dense         dense_path(600) on the golden map
      bind-<k>      the four bindings of the one-handle test: 4 096 / 614, 4 097 / 615, 4 095 / 153, 4 096 / 614 again"""
    if name in _CASES:
        return _CASES[name]
    kind, _, arg = name.partition("-")
    if kind == "path":
        world = golden_world()
        c = Case(name, world, limit_path(int(arg), world, spacing=0.06), seed=int(arg))
    elif kind == "map":
        world = limit_map(oracle, int(arg), seed=int(arg) % 7)
        c = Case(name, world, limit_path(154, world), seed=int(arg))
    elif name == "max-delays":
        world = limit_map(oracle, 4096, seed=1)
        c = Case(name, world, limit_path(614, world), delays=dict(control_delay=2, pose_delay=1, state_delay=3), timeout=20, seed=1)
    elif name == "max-diffdrive":
        world = limit_map(oracle, 4096, verts=F.DIFFDRIVE, seed=2)
        c = Case(name, world, limit_path(614, world), model="diffdrive", noisy=False, seed=2)
    elif name == "max-wide":
        verts = F.TRICYCLE * WIDE_SCALE
        assert F.footprint_is_wide(verts, WIDE_RES) and F.check_kernel_size(verts, WIDE_RES)
        world = limit_map(oracle, 4096, verts=verts, res=WIDE_RES, seed=3)
        c = Case(name, world, limit_path(154, world, spacing=0.06), footprint_scale=WIDE_SCALE, seed=3, v_scale=3.0)
    elif name == "dense":
        world = golden_world()
        c = Case(name, world, dense_path(600, world), seed=4, xy_sigma=0.05, th_sigma=0.15, v_min=0.2, early=0.6, target_back=200)
    elif kind == "bind":
        words, n_way = ((4096, 614), (4097, 615), (4095, 153), (4096, 614))[int(arg)]
        world = limit_map(oracle, words, seed=5)
        c = Case(name, world, limit_path(n_way, world), seed=5, steps=12)
    else:
        raise KeyError(name)
    assert not oracle.pose_collides(c.path[0, 0], c.path[0, 1], c.path[0, 2], world["verts"], c.cm, c.origin, c.res), name
    _CASES[name] = c
    return c


STEP_CASES = (["path-%d" % n for n in PATH_LENGTHS] + ["map-%d" % w for w in (2305, 4095, 4096, 4097)] +
              ["max-delays", "max-diffdrive", "max-wide", "dense"])
BIND_CASES = ["bind-%d" % k for k in range(4)]


# ---- the oracle's run -------------------------------------------------------------------------------------------------------------
def load_oracle(oracle, c):
    """an OracleBatch on the case's world, at its start states"""
    ref = oracle.OracleBatch(c.oracle_params(oracle), N, c.cm, c.origin, c.res, c.path)
    ref.reset_from_paths()
    st, md, tgt, it = c.start
    for f in range(7):
        ref.st[f][:] = st[f]
    ref.min_dist[:], ref.target_idx[:], ref.cur_iter[:] = md, tgt, it
    ref.obs_pose[:] = np.stack(ref.st[:3], axis=1)
    ref.obs_state[:] = np.stack(ref.st, axis=1)
    return ref


def run_oracle(oracle, c, z=None):
    """The case's steps, fed the normals `z` (one [N, 3] per step; None: the case's own host-drawn ones) -> per step a dict of
    what the step left (robot [7, N], min_dist, target_idx, current_iter, robot_collided, reward, done, collided_now) and what
    it started from (pre_robot, pre_target, pre_iter)"""
    ref = load_oracle(oracle, c)
    if z is None:
        z = c.host_z
    rows = []
    for t, a in enumerate(c.actions):
        pre = dict(pre_robot=np.stack(ref.st), pre_target=ref.target_idx.copy(), pre_iter=ref.cur_iter.copy())
        ref.step(a.astype(np.float64), z[t] if c.noisy else None, auto_reset=True, threads=8)
        rows.append(dict(pre, robot=np.stack(ref.st), min_dist=ref.min_dist.copy(), target_idx=ref.target_idx.copy(),
                         current_iter=ref.cur_iter.copy(), robot_collided=ref.collided.copy(), reward=ref.reward.copy(),
                         done=ref.done.copy(), collided_now=ref.collided_now.copy(), z=z[t] if c.noisy else None,
                         obs_pose=ref.obs_pose.copy(), obs_state=ref.obs_state.copy()))
    return rows


def path_conditions(c, rows):
    """-> (envs whose target_idx was n_way - 1 or more after some step, episodes that ended at the goal, envs that were reset).
    An episode ends for a collision, at the time-out or at the goal (target_idx > n_way - 1, which the auto-reset has replaced
    by the time the step returns): the ends that were neither of the first two are counted."""
    at_tail = np.zeros(N, dtype=bool)
    was_reset = np.zeros(N, dtype=bool)
    goals = 0
    for r in rows:
        at_tail |= r["target_idx"] >= c.n_way - 1
        done = r["done"] != 0
        was_reset |= done
        goals += int((done & (r["collided_now"] == 0) & (r["pre_iter"] + 1 < c.timeout)).sum())
    return int(at_tail.sum()), goals, int(was_reset.sum())


def map_conditions(oracle, c, rows):
    """Over the colliding poses of the run: (how many cover a listed speckle of the bitmap's last 768 words, how many cover one
    of words 2 304 .. 3 071).  The colliding pose is the one the robot model gives from the state before the step (the step
    itself rolls it back); with a control queue the command is not the step's own, and the pose the robot was rolled back to
    stands in -- less than a pixel away (0.5 m/s for 0.05 s)."""
    verts, res = np.asarray(c.world["verts"]), c.res
    speck = np.zeros(c.cm.shape, dtype=bool)
    speck[c.world["speckles"]] = True
    words = word_of(c.cm.shape)
    p = c.oracle_params(oracle)
    in_tail = in_fourth = 0
    for t, r in enumerate(rows):
        for i in np.nonzero(r["collided_now"])[0]:
            if c.delays:
                pose = r["pre_robot"][:3, i]
            else:
                pose = oracle.robot_step(p, r["pre_robot"][:, i], c.actions[t][i].astype(np.float64),
                                         r["z"][i] if c.noisy else None)[0][:3]
            img = oracle.pixel_footprint(pose[2], verts, res) != 0
            px = oracle.world_to_pixel(pose[:2], c.origin, res)
            ky, kx = np.nonzero(img)
            rr, cc = px[1] + ky - img.shape[0] // 2, px[0] + kx - img.shape[1] // 2
            ok = (rr >= 0) & (rr < c.cm.shape[0]) & (cc >= 0) & (cc < c.cm.shape[1])
            hit = words[rr[ok], cc[ok]][speck[rr[ok], cc[ok]]]
            in_tail += int((hit >= c.words - STAGERS).any())
            in_fourth += int(((hit >= FOURTH_SLICE) & (hit < FOURTH_SLICE + STAGERS)).any())
    return in_tail, in_fourth


def scan_candidates(oracle, c, rows, steps=8):
    """For each of the first `steps` steps and every block of 64 consecutive envs: the sum over the block's envs of
    last_reached - max(target_idx, first way point within goal_spat_dist of the pose) + 1, from oracle.find_last_reached for the
    pose after the step and the target before it; envs that reach nothing, and envs whose episode ended in the step (their pose
    is the reset one), add nothing.  Any correct contiguous candidate window holds at least these way points.  -> int [steps, blocks]"""
    blocks = -(-N // 64)
    out = np.zeros((steps, blocks), dtype=np.int64)
    for t in range(steps):
        r = rows[t]
        for i in range(N):
            if r["done"][i]:
                continue
            pose = r["robot"][:3, i]
            last = oracle.find_last_reached(pose, c.path, SP, AP)
            if last is None:
                continue
            within = np.nonzero(np.hypot(c.path[:, 0] - pose[0], c.path[:, 1] - pose[1]) < SP)[0]
            out[t, i // 64] += last - max(int(r["pre_target"][i]), int(within[0])) + 1
    return out
