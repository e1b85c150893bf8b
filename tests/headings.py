"""Headings outside [-pi, pi): the batches that carry them into the moving kernels.  Built on tests/offstock.Batch (600 envs =
two 256-env workgroups and a tail, 32 steps): the path angles of way points j >= 1 are shifted by whole turns, and on every
third step the robot headings are written anew -- the same doubles into the oracle's st[2] and, by the GPU tests, into
env.state.robot[2].
  'wrapped'  0 / +1 / -1 turn, never onto 3 pi: the reference steps such a heading normally (one exact add or subtract in
             py_mod_two_pi's second branch), no error word anywhere;
  'jumping'  0, +-2, +-3, +-50 turns and the knife edge +-(3 pi - U(0, 5e-3)): path_velocity raises in the reference (the
             oracle's err = 1) for every heading two turns or more away, and on the knife edge exactly when the step carries
             the heading across 3 pi -- which depends on the command.
tests/test_headings_host.py steps the batches on the CPU oracle alone and asserts that they are not vacuous;
tests/test_gpu_headings.py steps them on the GPU and on the oracle side by side and asserts the same floors on its own runs.
oracle/gen_golden.py imports TURNS and shift_path for tests/golden/g17_headings.npz."""
import numpy as np

import lookahead_ref as LR
import offstock as OS

TWO_PI = 2.0 * np.pi
TURNS = np.array([0, 1, -1, 2, -2, 3, 50, -1000])    # way point j >= 1 is shifted by TURNS[j % 8] turns
FAR_TURNS = np.array([2, -2, 3, -3, 50, -50])
KNIFE_WIDTH = 5e-3
# 'wrapped' keeps this far from +-3 pi: a step turns the robot by |w| dt <= 2 * (max_front_wheel_speed / 2) / 0.964 * 0.1 =
# 0.11 rad (the fastest command of the batches below, noise aside), and a heading that crosses 3 pi within the step is flagged
KEEP_OFF = 0.25
INJECT_EVERY = 3
WORLDS = [("mini", 1), ("aisle", 7)]     # (world, row of offstock.ROWS): shared path in LDS / private paths and the prefilter
NONE, LEGAL, FAR, KNIFE = 0, 1, 2, 3


def shift_path(path):
    """path [m, 3] or [n, m, 3] with the angle of way point j >= 1 shifted by TURNS[j % 8] turns; path[0] (the start heading
    after a reset) stays"""
    out = np.array(path, dtype=np.float64)
    j = np.arange(out.shape[-2])
    out[..., 1:, 2] += TURNS[j[1:] % 8] * TWO_PI
    return out


def inject(rng, th, kind, thirds=False):
    """New headings for the headings th [n] -> (new headings, category [n]).  'wrapped': a third each 0 / +1 / -1 turn, the
    sign turned round where the result would come within KEEP_OFF of +-3 pi.  'jumping': 40 % untouched, 30 % shifted by one of
    FAR_TURNS, 30 % replaced by +-(3 pi - U(0, KNIFE_WIDTH)); thirds (the planner scenarios): a third on the knife edge, a
    third at +-1 turn, the rest at FAR_TURNS."""
    n = len(th)
    th = np.asarray(th, dtype=np.float64)
    new, cat = th.copy(), np.zeros(n, np.int32)
    if kind == "wrapped":
        k = rng.randint(-1, 2, n)
        out = th + k * TWO_PI
        k = np.where(np.abs(out) > 3 * np.pi - KEEP_OFF, -k, k)
        new = th + k * TWO_PI
        cat[k != 0] = LEGAL
        assert (np.abs(new) <= 3 * np.pi - KEEP_OFF).all()
        return new, cat
    assert kind == "jumping"
    u = rng.rand(n)
    if thirds:
        cat[:] = np.where(np.arange(n) % 3 == 0, KNIFE, np.where(np.arange(n) % 3 == 1, LEGAL, FAR))
    else:
        cat[:] = np.where(u < 0.4, NONE, np.where(u < 0.7, FAR, KNIFE))
    far = FAR_TURNS[rng.randint(0, len(FAR_TURNS), n)]
    one = rng.choice([-1, 1], n)
    edge = rng.choice([-1.0, 1.0], n) * (3 * np.pi - rng.uniform(0, KNIFE_WIDTH, n))
    new = np.where(cat == FAR, th + far * TWO_PI, new)
    new = np.where(cat == LEGAL, np.where(np.abs(th + one * TWO_PI) > 3 * np.pi - KEEP_OFF, th - one * TWO_PI, th + one * TWO_PI), new)
    new = np.where(cat == KNIFE, edge, new)
    assert (np.abs(new) <= 51 * TWO_PI).all()    # (the float32 heading of the prefilter holds its bound below 2048 rad)
    return new, cat


class Batch(OS.Batch):
    """offstock.Batch of `world` on grid row `row` with shifted path angles (shifted = False: the same batch -- start states,
    actions, injections -- on the path as recorded) and the heading injection `kind`."""

    def __init__(self, oracle, world, row, kind, shifted=True, n=OS.N_ENVS):
        OS.Batch.__init__(self, oracle, world, row, n=n)
        self.kind = kind
        self.inject_rng = np.random.RandomState(self.seed + 7000)
        if shifted:
            self.paths = shift_path(self.paths)
            if world == "aisle":
                self.templates = [dict(g, path=shift_path(g["path"])) for g in self.templates]
            self.ref = oracle.OracleBatch(self.cfg.oracle_params(oracle), n, self.maps, self.origins, self.res, self.paths, lens=self.lens)
            self.ref.reset_from_paths()
            st, md, tgt, it = self.start
            for f in range(7):
                self.ref.st[f][:] = st[f]
            self.ref.min_dist[:], self.ref.target_idx[:], self.ref.cur_iter[:] = md, tgt, it
        self.counts.update(outside=0, flagged=0, knife_flagged=0, knife_unflagged=0)
        self.category = np.zeros(n, np.int32)

    def injection(self):
        """Before step self.t: None, or on every third step the new headings [n], already written into the oracle's st[2]"""
        self.category[:] = NONE
        if self.t % INJECT_EVERY:
            return None
        new, self.category = inject(self.inject_rng, self.ref.st[2], self.kind)
        self.ref.st[2][:] = new
        return new

    def step_oracle(self, actions, z=None, count_drawn=False):
        self.counts["outside"] += int((np.abs(self.ref.st[2]) > np.pi).sum())
        OS.Batch.step_oracle(self, actions, z, count_drawn)
        flagged = self.ref.err != 0
        self.counts["flagged"] += int(flagged.sum())
        self.counts["knife_flagged"] += int((flagged & (self.category == KNIFE)).sum())
        self.counts["knife_unflagged"] += int((~flagged & (self.category == KNIFE)).sum())

    def assert_floors(self):
        c = self.counts
        tag = "%s row %d %s: %s" % (self.world, self.row, self.kind, c)
        assert c["done"] >= 20 and c["collided"] >= 20 and c["advanced"] >= 10, tag
        if self.kind == "wrapped":
            assert c["outside"] >= 2000 and c["flagged"] == 0, tag
        else:
            assert c["flagged"] >= 300 and c["knife_flagged"] >= 50 and c["knife_unflagged"] >= 50, tag


# ---- the planner scenarios ------------------------------------------------------------------------------------------
PLAN_N, PLAN_H = 96, 8
PLAN_WORLDS = [("mini", 11), ("aisle", 11)]


def planning_start(oracle, world, row, warm=6):
    """A live batch of PLAN_N envs (offstock.Batch stepped `warm` times on the oracle, no noise in the planners' forward model),
    then a 'jumping' injection by thirds -> (batch, StartState, oracle world dict, noise-free oracle params, category [n]).
    The knife-edge envs get their heading the way a reset gives one: on a robot at rest with a straight wheel (v = w = steering
    command = wheel angle = 0).  The dynamic model lets one command change w by at most max_angular_acceleration * dt and the
    wheel angle by at most max_front_wheel_speed * dt, so a robot that already turns crosses 3 pi or stays off it whatever the
    candidate says; from rest the candidate's steering decides the side and its speed the reach.  Row 11 of the grid (dt 0.1,
    the short robot with its 2 rad/s^2) is the one where a step from rest reaches across the whole knife edge: on the oracle
    every knife-edge env then holds flagged and unflagged candidates (tests/test_headings_host.py asserts at least half)."""
    b = Batch(oracle, world, row, "jumping", n=PLAN_N)
    for _ in range(warm):
        b.step_oracle(b.next_actions())
    ref = b.ref
    new, cat = inject(b.inject_rng, ref.st[2], "jumping", thirds=True)
    robot = np.stack(ref.st)
    robot[2] = new
    robot[3:7, cat == KNIFE] = 0.0
    start = LR.StartState(robot, ref.min_dist.copy(), ref.target_idx.copy(), ref.cur_iter.copy(), ref.collided.copy())
    world_d = dict(costmaps=b.maps, origins=b.origins, resolution=b.res, paths=b.paths, lens=b.lens)
    return b, start, world_d, b.cfg.oracle_params(oracle, noise=False), cat


def box_library(rng, shape):
    """commands drawn from the action box of PlanEnv, float32, held over the horizon: shape (K,) -> [H, K, 2] shared,
    (N, K) -> [H, N, K, 2] per env"""
    box = OS.action_box()
    cmd = rng.uniform(box.low, box.high, tuple(shape) + (2,)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(cmd, (PLAN_H,) + cmd.shape))


def mixed_share(err, cat):
    """share of the knife-edge envs whose candidates (err [N, K]) are neither all flagged nor all unflagged"""
    flagged = np.asarray(err)[cat == KNIFE] != 0
    return float((flagged.any(axis=1) & ~flagged.all(axis=1)).mean())


MPPI = dict(sigma=(0.2, 0.8), iterations=2, lam=0.3, penalty=2.0)


def plan_mean(start):
    """the initial MPPI plan [N, H, 2]: 0.4 m/s, steering 1.4 rad AWAY from the side the heading's sign names -- on the knife
    edge only a perturbation beyond 1.75 sigma steers across 3 pi, so flagged candidates are few: some envs hold none, some a
    single one, some only odd-numbered ones (what a group reduction that leaves lanes out would lose)"""
    mean = np.zeros((start.n, PLAN_H, 2))
    mean[..., 0] = 0.4
    mean[..., 1] = (-1.4 * np.sign(start.robot[2]))[:, None]
    return mean


def rare_flags(iter_err, cat):
    """iter_err [I, N, K] -> over the knife-edge envs: (flagged envs, envs with exactly one flagged candidate, envs whose flagged
    candidates all carry odd numbers)"""
    e = (np.asarray(iter_err) != 0).any(axis=0)[cat == KNIFE]
    count = e.sum(axis=1)
    return int((count > 0).sum()), int((count == 1).sum()), int((e[:, 1::2].any(axis=1) & ~e[:, 0::2].any(axis=1)).sum())
