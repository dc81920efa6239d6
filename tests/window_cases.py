"""Drives of the persistent window (lvf_window_*) at the sizes where its device-side assembly takes its size-dependent paths, each
with a python MIRROR of the window that is the input of tests/window_ref.assemble.

A case is a generator of steps over a Mirror (`drive`): the generator applies the front end's events to the mirror (which logs them for
whoever feeds the same events to a real window) and yields `dict(kind="solve", iters=, check_cost=, label=)` when the window is to be
solved, `dict(kind="reject", max_px=)` when the outlier gate is to run.  `play` runs a drive; without a real window behind it (the
DRY RUN every case constructor makes) a tick with iterations puts the case's noise-free state into the mirror (`dry_solve`: where a solve
is heading) and the gate's choice is taken from the mirror's own reprojection errors.  What a case is FOR — its conditions — is asserted at construction from the dry run's per-tick figures, before any GPU call.

Those figures follow the sizing rules of lvf_window's assemble_device (window.hip), restated in Mirror.tick:
  * feature arena: a keyframe with n features that has no segment, or outgrew its own, takes a new one of n + n/4 + 64 elements at the
    arena's end; when that would pass the arena's capacity everything is laid out again ("re-layout") in an arena of at least
    max(2 * sum of those capacities, 4096) elements;
  * landmark table: 64 bytes per entry of the table (+ 16), entries freed by the pruning are re-used last-freed-first;
  * a device buffer that has to grow is allocated a quarter (+ 16) larger than asked and loses its content (DevBuf::ensure)."""
import numpy as np

from lvio_fusion_amd import synthetic as syn
from tests import window_ref as ref

KF_ID0, LM_ID0 = 2 ** 40, 2 ** 41


def unit_cameras(cfg):
    """the camera extrinsics with UNIT quaternions (the 7-digit matrices of the rig give |q| - 1 = 2.7e-7, which every restatement of
    q p q^-1 would see differently)"""
    out = []
    for cam in ("cam0", "cam1"):
        c = dict(cfg[cam]); e = np.array(c["extrinsic"], np.float64); e[:4] /= np.linalg.norm(e[:4]); c["extrinsic"] = e
        out.append(c)
    return out


class Mirror:
    """What lvf_window keeps on the host, as arrays: the active keyframes, the landmark TABLE (entries are re-used, never moved) and the
    features per keyframe."""

    def __init__(self, left, right, baseline, weak_thr, capacity):
        self.left, self.right, self.baseline, self.weak_thr = left, right, baseline, weak_thr
        self.kf = []                                     # active keyframe ids, ascending
        self.pose, self.vel, self.ba, self.bg, self.w, self.good, self.pre = {}, {}, {}, {}, {}, {}, {}
        self.obs = {}                                    # keyframe id -> dict(id [n], idx [n] (table index), xy [n][2])
        self.n_tab = 0
        self.T_id = np.zeros(capacity, np.int64); self.T_birth = np.zeros(capacity, np.int64); self.T_right = np.zeros((capacity, 2))
        self.T_invd = np.zeros(capacity); self.T_fixed = np.zeros(capacity, bool); self.T_pw = np.zeros((capacity, 3))
        self.T_alive = np.zeros(capacity, bool)
        self.index, self.free, self.departed, self.ever_departed = {}, [], {}, []
        self.dirty = set()
        self.log = []
        self.seg_cap, self.arena_end, self.arena_cap, self.lmtab_cap, self.ticks_done = {}, 0, 0, 0, 0
        self.stats = []

    # ---- the front end's entries (lvf_window_add_keyframe, _set_imu, _add_landmark, _add_observation, _remove_observation, _slide)
    def add_keyframe(self, kid, pose, w):
        assert not self.kf or kid > self.kf[-1]
        self.kf.append(kid); self.pose[kid] = np.array(pose, np.float64); self.w[kid] = float(w); self.good[kid] = False; self.pre[kid] = None
        self.obs[kid] = dict(id=np.zeros(0, np.int64), idx=np.zeros(0, np.int64), xy=np.zeros((0, 2))); self.seg_cap[kid] = 0
        self.log.append(("kf", kid, self.pose[kid], self.w[kid]))

    def set_imu(self, kid, vel, ba, bg, pre):
        """pre: which pre-integration (an index the case's `imu` list understands) or None"""
        self.vel[kid], self.ba[kid], self.bg[kid] = (np.array(x, np.float64) for x in (vel, ba, bg))
        self.good[kid] = True; self.pre[kid] = pre
        self.log.append(("imu", kid, self.vel[kid], self.ba[kid], self.bg[kid], pre))

    def _append(self, kid, ids, idx, xy):
        o = self.obs[kid]
        assert len(np.intersect1d(o["id"], ids)) == 0 and len(np.unique(ids)) == len(ids), "one feature per (keyframe, landmark)"
        o["id"] = np.concatenate([o["id"], ids]); o["idx"] = np.concatenate([o["idx"], idx]); o["xy"] = np.concatenate([o["xy"], xy])

    def add_landmarks(self, kid, ids, left_ob, right_ob, inv_depth):
        ids = np.asarray(ids, np.int64); left_ob = np.asarray(left_ob, np.float64).reshape(-1, 2); right_ob = np.asarray(right_ob, np.float64).reshape(-1, 2)
        inv_depth = np.asarray(inv_depth, np.float64).reshape(-1)
        kid = np.broadcast_to(np.asarray(kid, np.int64), ids.shape)       # (one birth keyframe for all, or one each: the table fills in call order)
        idx = np.zeros(len(ids), np.int64)
        for j, i in enumerate(ids.tolist()):
            assert i not in self.index
            if self.free:
                at = self.free.pop()
            else:
                at = self.n_tab; self.n_tab += 1
            idx[j] = at; self.index[i] = at
        self.T_id[idx] = ids; self.T_birth[idx] = kid; self.T_right[idx] = right_ob; self.T_invd[idx] = inv_depth
        self.T_fixed[idx] = False; self.T_pw[idx] = 0.0; self.T_alive[idx] = True
        self.dirty.update(idx.tolist())
        for k in np.unique(kid).tolist():
            sel = kid == k
            self._append(k, ids[sel], idx[sel], left_ob[sel])
        if len(ids):
            self.log.append(("lm", kid.copy(), ids, left_ob, right_ob, inv_depth))

    def known(self, ids):
        return np.fromiter((i in self.index for i in np.asarray(ids, np.int64).tolist()), bool, len(ids))

    def add_observations(self, kid, ids, xy):
        ids = np.asarray(ids, np.int64); xy = np.asarray(xy, np.float64).reshape(-1, 2)
        idx = np.fromiter((self.index[i] for i in ids.tolist()), np.int64, len(ids))
        assert np.all(self.T_birth[idx] < kid)
        self._append(kid, ids, idx, xy)
        if len(ids):
            self.log.append(("ob", kid, ids, xy))

    def _drop(self, kid, ids):
        o = self.obs[kid]
        keep = ~np.isin(o["id"], ids)
        o["id"], o["idx"], o["xy"] = o["id"][keep], o["idx"][keep], o["xy"][keep]

    def remove_observations(self, kid, ids):
        ids = np.asarray(ids, np.int64)
        self._drop(kid, ids)                                   # (no pruning: a landmark nobody observes stays known until the next slide)
        if len(ids):
            self.log.append(("rm", kid, ids))

    def slide(self, first_id):
        self.log.append(("slide", first_id))
        drop = [k for k in self.kf if k < first_id]
        if not drop:
            return
        for k in drop:
            self.departed[k] = self.pose[k].copy(); self.ever_departed.append(k)
        n = self.n_tab
        rows = np.flatnonzero(self.T_alive[:n] & ~self.T_fixed[:n] & (self.T_birth[:n] < first_id))
        if len(rows):      # the world point freezes at the departing birth keyframe's last pose and the landmark's last inverse depth
            bp = np.array([self.departed[b] for b in self.T_birth[rows].tolist()])
            self.T_pw[rows] = ref.to_world(self.right, self.T_right[rows], self.T_invd[rows], bp)
            self.T_fixed[rows] = True
            self.dirty.update(rows.tolist())
        self.kf = [k for k in self.kf if k >= first_id]
        for k in drop:
            del self.obs[k]; del self.seg_cap[k]
        self.prune()

    def prune(self):
        """landmarks no active keyframe observes leave (their table entries become free, in ascending order); departed poses stay only while
        a live landmark was born there"""
        n = self.n_tab
        seen = np.zeros(n, bool)
        for k in self.kf:
            seen[self.obs[k]["idx"]] = True
        gone = np.flatnonzero(self.T_alive[:n] & ~seen)
        for at in gone.tolist():
            del self.index[int(self.T_id[at])]
        self.T_alive[gone] = False; self.T_fixed[gone] = False
        self.free.extend(gone.tolist()); self.dirty.update(gone.tolist())
        anchors = set(self.T_birth[:n][self.T_alive[:n]].tolist())
        self.departed = {k: p for k, p in self.departed.items() if k in anchors}

    # ---- what a real window reports back
    def apply_removed(self, pairs):
        """(landmark id, keyframe id) pairs the outlier gate removed (lvf_window_reject_outliers prunes when it removed anything)"""
        by_kf = {}
        for l, k in pairs:
            by_kf.setdefault(k, []).append(l)
        for k, ls in by_kf.items():
            self._drop(k, np.array(ls, np.int64))
        if pairs:
            self.prune()

    def take_state(self, pose, imu, inv_depth):
        """the solved state of a real window: pose(kf id), imu(kf id) -> (vel, ba, bg), inv_depth(landmark id)"""
        for k in self.kf:
            self.pose[k] = np.array(pose(k), np.float64)
            if self.good[k]:
                self.vel[k], self.ba[k], self.bg[k] = (np.array(x, np.float64) for x in imu(k))
        for i, at in self.index.items():
            self.T_invd[at] = inv_depth(i)

    def take_log(self):
        ev, self.log = self.log, []
        return ev

    # ---- views
    def n_features(self):
        return sum(len(self.obs[k]["id"]) for k in self.kf)

    def live_ids(self):
        return sorted(self.index)

    def ref_input(self):
        rows = np.flatnonzero(self.T_alive[:self.n_tab])
        row_of = np.full(max(self.n_tab, 1), -1, np.int64); row_of[rows] = np.arange(len(rows))
        kf = dict(id=np.array(self.kf, np.int64), pose=np.array([self.pose[k] for k in self.kf]), w_visual=np.array([self.w[k] for k in self.kf]),
                  good_imu=np.array([self.good[k] for k in self.kf]), has_pre=np.array([self.pre[k] is not None for k in self.kf]))
        lm = dict(id=self.T_id[rows], index=rows, birth=self.T_birth[rows], right_ob=self.T_right[rows], inv_depth=self.T_invd[rows],
                  fixed=self.T_fixed[rows], pw=self.T_pw[rows])
        okf = np.concatenate([np.full(len(self.obs[k]["id"]), p, np.int64) for p, k in enumerate(self.kf)])
        oidx = np.concatenate([self.obs[k]["idx"] for k in self.kf])
        assert np.all(row_of[oidx] >= 0), "a feature of a landmark that left"
        return kf, lm, dict(kf=okf, lm=row_of[oidx], xy=np.concatenate([self.obs[k]["xy"] for k in self.kf]))

    def assemble(self):
        kf, lm, obs = self.ref_input()
        out = ref.assemble(self.left, self.right, self.baseline, self.weak_thr, kf, lm, obs)
        out["used_index"] = lm["index"][out["slot_lm"]]
        return out

    def cpu_outliers(self, max_px):
        """the gate's rule on the mirror's own state: features that are not their landmark's first observation and re-project more than
        max_px away (the dry run's stand-in for lvf_window_reject_outliers)"""
        out = []
        for k in self.kf:
            o = self.obs[k]
            sel = self.T_birth[o["idx"]] != k
            idx = o["idx"][sel]
            if not len(idx):
                continue
            pw = self.T_pw[idx].copy()
            live = ~self.T_fixed[idx]
            if live.any():
                bp = np.array([self.pose[b] for b in self.T_birth[idx[live]].tolist()])
                pw[live] = ref.to_world(self.right, self.T_right[idx[live]], self.T_invd[idx[live]], bp)
            px, _ = syn.project(self.left, self.pose[k][None], pw)
            bad = np.linalg.norm(px - o["xy"][sel], axis=1) > max_px
            out += [(int(l), k) for l in o["id"][sel][bad].tolist()]
        return out

    def tick(self, asm, label):
        """one device-assembly tick's bookkeeping (see the module docstring for the rules) -> a record in self.stats"""
        n = {k: len(self.obs[k]["id"]) for k in self.kf}
        cap_of = lambda c: c + c // 4 + 64
        grow = [k for k in self.kf if self.seg_cap[k] < n[k]]
        moved = [k for k in grow if self.seg_cap[k] > 0]
        relayout = self.arena_end + sum(cap_of(n[k]) for k in grow) > self.arena_cap
        if relayout:
            want = max(2 * sum(cap_of(n[k]) for k in self.kf), 4096)
            if want > self.arena_cap:
                self.arena_cap = want + want // 4 + 16
            self.arena_end = 0
            for k in self.kf:
                self.seg_cap[k] = 0
            moved = []
        for k in self.kf:
            if self.seg_cap[k] < n[k]:
                self.seg_cap[k] = cap_of(n[k]); self.arena_end += self.seg_cap[k]
        need = 64 * self.n_tab + 16
        realloc = need > self.lmtab_cap
        if realloc:
            self.lmtab_cap = need + need // 4 + 16
        resident = self.ticks_done > 0 and not realloc
        hole = np.ones(self.n_tab, bool); hole[asm["used_index"]] = False          # free, or alive and in PoseOnly blocks only
        self.stats.append(dict(label=label, n_tab=self.n_tab, holes_below_1024=int(hole[:1024].sum()), holes_from_1024=int(hole[1024:].sum()),
                               holes_below_16384=int(hole[:16384].sum()), holes_from_16384=int(hole[16384:].sum()),
                               relayout=relayout, first=self.ticks_done == 0, moved=len(moved), dirty=len(self.dirty), resident=resident,
                               realloc_while_resident=self.ticks_done > 0 and realloc, free=len(self.free), features=self.n_features(),
                               counts=dict(asm["counts"]), frame_sizes=[n[k] for k in self.kf]))
        self.dirty = set()
        self.ticks_done += 1


def play(case, mirror, actor=None):
    """runs case.drive over `mirror`; `actor` (the GPU test) feeds each step's events to real windows: actor.solve(step, events, asm),
    actor.reject(step, events) -> the removed (landmark id, keyframe id) pairs"""
    for step in case.drive(mirror):
        ev = mirror.take_log()
        if step["kind"] == "solve":
            asm = mirror.assemble()
            mirror.tick(asm, step["label"])
            if actor is not None:
                actor.solve(step, ev, asm)
            elif step["iters"] > 0:
                case.dry_solve(mirror)
        else:
            removed = actor.reject(step, ev) if actor is not None else mirror.cpu_outliers(step["max_px"])
            mirror.apply_removed(removed)


class Case:
    weak_thr = 20
    with_imu = True

    def mirror(self):
        return Mirror(self.left, self.right, syn.baseline(), self.weak_thr, self.capacity)

    def check(self):
        m = self.mirror()
        play(self, m)
        self.conditions(m.stats)
        return m.stats

    def new_keyframe(self, m, t):
        cfg = self.cfg
        m.add_keyframe(KF_ID0 + t, cfg["poses"][t], cfg["w_kf"][t])
        if self.with_imu:
            m.set_imu(KF_ID0 + t, cfg["vel"][t], cfg["ba"][t], cfg["bg"][t], t - 1 if t > 0 else None)

    def imu_frame(self, i):
        return self.cfg["imu"][i]

    def dry_solve(self, m):
        pass


def solve_step(label, iters=0, check_cost=True):
    return dict(kind="solve", label=label, iters=iters, check_cost=check_cost)


class Tiles(Case):
    """A 40-tick drive through an 8-keyframe window at a few tiles: ~300 landmarks born and ~2000 re-observed per keyframe (the landmark
    table passes 1024 entries after four ticks and holds 3-4 k in the steady state, ~20 k features = ~80 classify workgroups), with
      * keyframe EMPTY created without any feature: it is the last, a middle and the first keyframe of the window in turn;
      * keyframe BURST born with 4300 landmarks nobody observes again: the table grows past 8 k entries, and when that keyframe departs
        the slide frees them all at once — more than 4096 dirty records into a resident table — and leaves holes that later births fill
        last-freed-first;
      * at the ticks LATE + 3 a keyframe that is three ticks old receives the 45 % of its re-observations that were held back at its
        creation: more than its segment's slack, so it moves to the arena's end;
      * at the ticks TRIM removals bring the window's feature total to a multiple of 256, at the next tick to one more than that;
      * two iterations every 4th tick, and every 7th tick followed by the outlier gate (80 re-observations are gross outliers, 25-60 px off).
    Keyframe ids start at 2^40, landmark ids are a permutation offset by 2^41.  The conditions asserted below are counted by Mirror.tick
    with assemble_device's sizing rules (module docstring)."""
    W, TICKS, EMPTY, BURST, LATE, TRIM, N_BURST = 8, 40, 12, 22, (9, 28), (16, 37), 4300

    def __init__(self, with_imu, seed=811):
        self.with_imu = with_imu
        self.weak_thr = 20
        self.name = f"tiles-imu{int(with_imu)}"
        self.cfg = cfg = syn.config4_window(n_kf=self.TICKS, n_lm=300 * self.TICKS, n_prewindow=0, seed=seed, imu_samples=4)
        self.left, self.right = unit_cameras(cfg)
        extra = syn.config4_window(n_kf=2, n_lm=self.N_BURST, n_prewindow=0, seed=seed + 1, imu_samples=2)
        self.burst = dict(left=extra["tc"]["left_ob"], right=extra["tc"]["right_ob"], inv_depth=extra["inv_depth"])
        rng = np.random.default_rng(seed + 2)
        n_lm = cfg["n_lm"]
        perm = LM_ID0 + rng.permutation(n_lm + self.N_BURST)
        self.lm_id, self.burst_id = perm[:n_lm], perm[n_lm:]
        self.true_invd = np.zeros(len(perm)); self.true_invd[perm - LM_ID0] = np.concatenate([cfg["inv_depth_true"], extra["inv_depth_true"]])
        tf = cfg["tf"]
        self.tf_ob = tf["ob"].copy()
        bad = rng.choice(len(tf["lm_idx"]), 80, replace=False)
        self.tf_ob[bad] += rng.choice([-1, 1], (80, 2)) * rng.uniform(25, 60, (80, 2))
        self.held = rng.random(len(tf["lm_idx"])) < 0.45
        self.capacity = n_lm + self.N_BURST
        self.late_figures = []
        self.trim_figures = []
        self.stats = self.check()

    def drive(self, m):
        cfg = self.cfg
        tc, tf = cfg["tc"], cfg["tf"]
        self.late_figures, self.trim_figures = [], []
        for t in range(self.TICKS):
            kid = KF_ID0 + t
            self.new_keyframe(m, t)
            if t != self.EMPTY:
                born = np.flatnonzero(tc["kf_idx"] == t)
                l = tc["lm_idx"][born]
                m.add_landmarks(kid, self.lm_id[l], tc["left_ob"][born], tc["right_ob"][born], cfg["inv_depth"][l])
                rows = np.flatnonzero(tf["kf2_idx"] == t)
                if t in self.LATE:
                    rows = rows[~self.held[rows]]
                rows = rows[m.known(self.lm_id[tf["lm_idx"][rows]])]          # (a landmark whose features all left the window is gone)
                m.add_observations(kid, self.lm_id[tf["lm_idx"][rows]], self.tf_ob[rows])
            if t == self.BURST:
                m.add_landmarks(kid, self.burst_id, self.burst["left"], self.burst["right"], self.burst["inv_depth"])
            if t - 3 in self.LATE:
                old = KF_ID0 + t - 3
                rows = np.flatnonzero((tf["kf2_idx"] == t - 3) & self.held)
                rows = rows[m.known(self.lm_id[tf["lm_idx"][rows]])]
                before = len(m.obs[old]["id"])
                m.add_observations(old, self.lm_id[tf["lm_idx"][rows]], self.tf_ob[rows])
                self.late_figures.append(dict(tick=t, added=len(rows), slack=m.seg_cap[old] - before, position=m.kf.index(old), n_kf=len(m.kf)))
            m.slide(KF_ID0 + max(0, t - self.W + 1))
            if t in self.TRIM or t - 1 in self.TRIM:
                total = m.n_features()
                r = total % 256 if t in self.TRIM else (total - 1) % 256
                victim = max(m.kf[:-1], key=lambda k: int((m.T_birth[m.obs[k]["idx"]] != k).sum()))      # an older keyframe with features to spare
                o = m.obs[victim]
                cand = np.sort(o["id"][m.T_birth[o["idx"]] != victim])
                m.remove_observations(victim, cand[:r])
                self.trim_figures.append(dict(tick=t, features=m.n_features()))
            yield solve_step(f"{self.name} tick {t}", iters=2 if t % 4 == 3 or t % 7 == 6 else 0, check_cost=t % 5 == 0)
            if t % 7 == 6:
                yield dict(kind="reject", max_px=10.0)

    def dry_solve(self, m):
        for k in m.kf:
            m.pose[k] = self.cfg["poses_true"][k - KF_ID0].copy()
        at = np.fromiter(m.index.values(), np.int64, len(m.index))
        m.T_invd[at] = self.true_invd[m.T_id[at] - LM_ID0]

    def conditions(self, stats):
        assert len(stats) == self.TICKS
        assert max(s["n_tab"] for s in stats) > 1024, "the landmark table never passes one 1024-chunk"
        both = [s for s in stats if 0 < s["holes_below_1024"] < 1024 and 0 < s["holes_from_1024"] < s["n_tab"] - 1024]      # (partial on both sides)
        assert len(both) >= 5, f"only {len(both)} ticks with free or unused table entries on both sides of index 1024"
        relayouts = [s["label"] for s in stats if s["relayout"] and not s["first"]]
        assert len(relayouts) >= 3, f"arena re-layouts after the first tick: {relayouts}"
        assert any(min(s["counts"][k] for k in ("po", "tf", "tc")) > 0 for s in stats)
        assert len(self.late_figures) == 2
        for f in self.late_figures:
            assert f["added"] > f["slack"] >= 0 and 0 < f["position"] < f["n_kf"] - 1, f"late observations: {f}"
        assert sum(s["moved"] for s in stats) >= 1, "no keyframe ever moved to the arena's end"
        assert len(self.trim_figures) == 4
        for a, b in zip(self.trim_figures[0::2], self.trim_figures[1::2]):
            assert a["features"] % 256 == 0 and b["features"] % 256 == 1 and b["tick"] == a["tick"] + 1, f"{a} {b}"
        for p, t in (("last", self.EMPTY), ("middle", self.EMPTY + 3), ("first", self.EMPTY + self.W - 1)):
            sizes = stats[t]["frame_sizes"]
            at = dict(last=len(sizes) - 1, middle=len(sizes) - 4, first=0)[p]
            assert sizes[at] == 0 and len(sizes) == self.W and sum(1 for x in sizes if x == 0) == 1, f"the empty keyframe is not the {p} one at tick {t}"
        assert any(s["dirty"] > 4096 and s["resident"] for s in stats), "no tick sends more than 4096 dirty landmark records into a resident table"
        assert any(s["realloc_while_resident"] for s in stats), "the landmark table never outgrows its buffer after the first tick"
        assert any(s["free"] > 0 for s in stats[self.BURST + self.W + 1:]), "freed table entries were all re-used at once"
        if not self.with_imu:
            assert any(s["counts"]["prior"] > 0 for s in stats)


class Long(Case):
    """64 active keyframes (kDaMaxKf: the device assembly's limit, every binary search over the keyframes at full depth) with ~60 features
    each: one tick at 64 keyframes, five ticks that each add a keyframe and slide by one (the steady state: one new segment, the dirty
    landmark records), then one tick after a feature was removed from the keyframes at positions 0, 31 and 63."""
    name = "long"

    def __init__(self, seed=606):
        self.cfg = cfg = syn.config4_window(n_kf=69, n_lm=69 * 12, n_prewindow=0, seed=seed, imu_samples=4, p_geom=0.2)
        self.left, self.right = unit_cameras(cfg)
        rng = np.random.default_rng(seed + 2)
        self.lm_id = LM_ID0 + rng.permutation(cfg["n_lm"])
        self.capacity = cfg["n_lm"]
        self.stats = self.check()

    def add_features(self, m, t):
        cfg = self.cfg
        tc, tf = cfg["tc"], cfg["tf"]
        born = np.flatnonzero(tc["kf_idx"] == t)
        l = tc["lm_idx"][born]
        m.add_landmarks(KF_ID0 + t, self.lm_id[l], tc["left_ob"][born], tc["right_ob"][born], cfg["inv_depth"][l])
        rows = np.flatnonzero(tf["kf2_idx"] == t)
        rows = rows[m.known(self.lm_id[tf["lm_idx"][rows]])]
        m.add_observations(KF_ID0 + t, self.lm_id[tf["lm_idx"][rows]], tf["ob"][rows])

    def drive(self, m):
        for t in range(64):
            self.new_keyframe(m, t); self.add_features(m, t)
        yield solve_step("long: 64 keyframes")
        for t in range(64, 69):
            self.new_keyframe(m, t); self.add_features(m, t)
            m.slide(KF_ID0 + t - 63)
            yield solve_step(f"long: slide {t - 63}")
        for p in (0, 31, 63):
            k = m.kf[p]
            o = m.obs[k]
            m.remove_observations(k, np.sort(o["id"])[len(o["id"]) // 2:][:1])
        yield solve_step("long: after removals at positions 0, 31, 63")

    def conditions(self, stats):
        assert len(stats) == 7 and all(s["counts"]["kf"] == 64 for s in stats)
        assert all(s["counts"]["imu"] == 63 for s in stats)
        mean = np.mean([np.mean(s["frame_sizes"]) for s in stats])
        assert 40 <= mean <= 90, f"{mean:.1f} features per keyframe"
        assert all(not s["relayout"] and s["resident"] for s in stats[2:6]), "the slides are not the steady state"
        assert any(min(s["counts"][k] for k in ("po", "tf", "tc")) > 0 for s in stats)


class Big(Case):
    """Past 512 classify workgroups (131 072 features: the second pass of k_da_scan's per-workgroup scan) and past 32 768 landmark table
    entries (three 16 k landmark passes), with holes.  N_LM = 33 000 is the smallest multiple of 1000 that meets both conditions at tick A
    (the table has one entry per landmark, so the table condition alone asks for more than 32 768 landmarks; the window then holds
    ~150 k features).  The landmarks enter in the order of their (permuted) ids, NOT keyframe by keyframe, so the table index says nothing
    about the birth keyframe and the entries that tick B leaves unused or free lie on both sides of index 16 384.
      A: 12 keyframes, everything but one keyframe's worth (1/12) of the re-observations of keyframes 4 .. 11, which is held back;
      B: after a slide to the 4th keyframe, with the held-back observations added."""
    name = "big"
    N_KF, N_LM = 12, 33000

    def __init__(self, seed=2121):
        self.cfg = cfg = syn.config4_window(n_kf=self.N_KF, n_lm=self.N_LM, n_prewindow=0, seed=seed, imu_samples=4)
        self.left, self.right = unit_cameras(cfg)
        rng = np.random.default_rng(seed + 2)
        self.lm_id = LM_ID0 + rng.permutation(cfg["n_lm"])
        tf = cfg["tf"]
        self.held = (tf["kf2_idx"] >= 4) & (rng.random(len(tf["lm_idx"])) < len(tf["lm_idx"]) / 12.0 / max(1, int((tf["kf2_idx"] >= 4).sum())))
        self.capacity = cfg["n_lm"]
        self.stats = self.check()

    def drive(self, m):
        cfg = self.cfg
        tc, tf = cfg["tc"], cfg["tf"]
        for t in range(self.N_KF):
            self.new_keyframe(m, t)
        order = np.argsort(self.lm_id[tc["lm_idx"]])
        l = tc["lm_idx"][order]
        m.add_landmarks(KF_ID0 + tc["kf_idx"][order].astype(np.int64), self.lm_id[l], tc["left_ob"][order], tc["right_ob"][order], cfg["inv_depth"][l])
        for t in range(self.N_KF):
            rows = np.flatnonzero((tf["kf2_idx"] == t) & ~self.held)
            m.add_observations(KF_ID0 + t, self.lm_id[tf["lm_idx"][rows]], tf["ob"][rows])
        yield solve_step("big A")
        m.slide(KF_ID0 + 3)
        for t in range(4, self.N_KF):
            rows = np.flatnonzero((tf["kf2_idx"] == t) & self.held)
            rows = rows[m.known(self.lm_id[tf["lm_idx"][rows]])]
            m.add_observations(KF_ID0 + t, self.lm_id[tf["lm_idx"][rows]], tf["ob"][rows])
        yield solve_step("big B")

    def conditions(self, stats):
        a, b = stats
        assert a["features"] > 131072 and a["n_tab"] > 32768, f"A: {a['features']} features, {a['n_tab']} table entries"
        assert a["counts"]["kf"] == 12 and b["counts"]["kf"] == 9
        assert b["n_tab"] > 16384
        assert b["holes_below_16384"] >= 1000 and b["holes_from_16384"] >= 1000, f"B: {b['holes_below_16384']} / {b['holes_from_16384']} unused or free entries"
        assert b["holes_below_16384"] < 16384 - 1000 and b["holes_from_16384"] < b["n_tab"] - 16384 - 1000, "B: a side of index 16 384 with (nearly) no used entry"
        assert b["features"] > 65536 and b["counts"]["po"] > 0 and b["free"] > 0


class Empty(Case):
    """No features: two keyframes with IMU and no landmark (no classify workgroup, an empty landmark table), a third keyframe with its
    landmarks, then every observation removed again (no workgroup, a table full of landmarks nobody uses)."""
    name = "empty"

    def __init__(self, seed=77):
        self.cfg = cfg = syn.config4_window(n_kf=3, n_lm=240, n_prewindow=0, seed=seed, imu_samples=4)
        self.left, self.right = unit_cameras(cfg)
        self.lm_id = LM_ID0 + np.random.default_rng(seed + 2).permutation(cfg["n_lm"])
        self.capacity = cfg["n_lm"]
        self.stats = self.check()

    def drive(self, m):
        cfg = self.cfg
        tc = cfg["tc"]
        self.new_keyframe(m, 0); self.new_keyframe(m, 1)
        yield solve_step("empty: two keyframes, no landmark")
        self.new_keyframe(m, 2)
        born = np.flatnonzero(tc["kf_idx"] == 2)
        l = tc["lm_idx"][born]
        m.add_landmarks(KF_ID0 + 2, self.lm_id[l], tc["left_ob"][born], tc["right_ob"][born], cfg["inv_depth"][l])
        yield solve_step("empty: a third keyframe with landmarks")
        m.remove_observations(KF_ID0 + 2, m.obs[KF_ID0 + 2]["id"].copy())
        yield solve_step("empty: every observation removed")

    def conditions(self, stats):
        a, b, c = stats
        assert a["features"] == 0 and a["n_tab"] == 0 and a["counts"]["imu"] == 1
        assert b["features"] > 0 and b["counts"]["tc"] == b["features"] and b["counts"]["lm"] == b["n_tab"]
        assert c["features"] == 0 and c["n_tab"] == b["n_tab"] and c["counts"]["lm"] == 0 and c["resident"]


def make(name):
    return dict(tiles_imu=lambda: Tiles(True), tiles_no_imu=lambda: Tiles(False), long=Long, big=Big, empty=Empty)[name]()


NAMES = ("tiles_imu", "tiles_no_imu", "long", "big", "empty")
