"""Pass lists of the cycle driver (``Mgrit.iteration`` / ``Mgrit._up``, core/mgrit.py): which intervals of a level one launch may
take (one rank, aligned ranks, a rank's share of a sharded level), what the closing C-point of every interval needs on the
coarser level, the boundary rows that travel between the exchange points of the reference (mgrit.py:693-713). Host logic only,
a mixin of ``Mgrit``. How it is put together:

  * ``OWN`` / ``_own(route)``: the methods a route stands for must be the library's own; one table, one test.
  * ``_whole_intervals`` (one rank, aligned ranks) and ``_rank_share`` (a rank of a sharded level): the two geometric tests.
  * one builder per route on top of them -- ``_coarse_down``, ``_coarse_down_rank``, ``_level_intervals``, ``_rank_intervals``
    (``_rank_intervals_up``), ``_gen_intervals`` --, each ``None`` (no such route on this level) or the route's lists, built once
    and kept by ``Mgrit._cached``: every call returns the same objects (the backend hangs device handles on them).
  * the exchange points that the passes move (``_x0``, ``_x0_relaxed``, ``_x4``, ``_head``) and the way up (``_up``)."""
import numpy as np

from pymgrit_amd.core.layout import IndexArray, as_index_array
from pymgrit_amd.core.options import options

# A fused route replaces calls of the driver's sweep methods by launches of its own: it is taken only while the methods it
# stands for are the library's (a subclass that overrides one keeps the sweep-by-sweep form, where its method runs). The
# sets are kept as they grew; where they differ:
#   _fas_residual_fused  every route but the whole-level pass (cf_fas / ec_relax_res stand for fas_residual as a whole)
#   _relax_f             routes that call f_relax for runs of their own (a rank's edge runs), the plan, which reorders its
#                        launches, and -- as found, no reason recorded -- the general passes
#   compute_residual     only where the residual sums are part of the pass (the whole-level and the general way up)
#   forward_solve        only where the coarsest level's solve itself is reordered or its input left unwritten
_SWEEPS = ("iteration", "f_relax", "c_relax", "fas_residual", "error_correction", "_exchange", "_ec_f_relax")
OWN = {
    'coarse_down': _SWEEPS + ("_fas_residual_fused",),
    'coarse_down_rank': _SWEEPS + ("_fas_residual_fused", "_relax_f"),
    'rank_intervals': _SWEEPS + ("_fas_residual_fused", "_relax_f"),
    'level_intervals': _SWEEPS + ("compute_residual",),
    'gen_intervals': _SWEEPS + ("compute_residual", "_fas_residual_fused", "_relax_f"),
    'plan': _SWEEPS + ("forward_solve", "_fas_residual_fused", "_relax_f"),      # Mgrit.plan_blocks
    'fuse_ec': ("error_correction", "f_relax", "fas_residual"),   # the kernel takes v_j from u_c: only the library's FAS sweep guarantees it
    'coarsest_u_unread': ("forward_solve",),
}


class RankSchedules:
    def _own(self, route) -> bool:
        """the methods that `route` stands for (OWN) are the library's, not a subclass's"""
        from pymgrit_amd.core.mgrit import Mgrit     # (late: mgrit.py imports this module)
        return all(getattr(type(self), name) is getattr(Mgrit, name) for name in OWN[route])

    def _detect_aligned(self) -> bool:
        """Several ranks whose shares of the time grid all END ON A C-POINT of every level (BASELINE configs 2-5 on 2 / 4 / 8
        ranks: nt - 1 a multiple of the rank count times every coarsening factor): a rank's local grid then looks
        like a one-rank grid -- slot 0 (the ghost point, a C-point of every level owned by the rank before) takes the place of
        the first time point, which nobody relaxes or corrects, and whole intervals follow. Such a rank runs the one-rank
        machinery (whole-level passes, C-point storage, pre-relaxed C-points, the planned cycle) with the exchange points of
        the reference refreshing slot 0 (ops 0 / 4 / 5; ops 1 / 2 / 3 / 7 never fire). Decided by all ranks together."""
        size, rank = self.comm_time_size, self.comm_time_rank
        if size == 1 or not getattr(self.backend, "device_links", False) or not self.global_conv_crit or \
                options.no_aligned:
            if size > 1 and getattr(self.backend, "device_links", False):
                self.comm_time.allgather_object(False)
            return False
        ok = self.lvl_max >= 2
        for lvl in range(self.lvl_max):
            if not ok:
                break
            n_own = len(self.index_local[lvl])
            ok = n_own >= 1 and (rank == 0 or (bool(self._ghost[lvl]) and self.get_from[lvl] == rank - 1)) and \
                (rank == size - 1 or self.send_to[lvl] == rank + 1) and (rank != 0 or self.get_from[lvl] < 0) and \
                (rank != size - 1 or self.send_to[lvl] < 0)
            if ok and lvl < self.lvl_max - 1:
                ok = (not self.comm_front[lvl] and not self.comm_back[lvl] and not self.first_is_c_point[lvl] and
                      not self.last_is_f_point[lvl] and len(self.index_local_c[lvl]) >= 1 and
                      bool(self._is_c_local[lvl][-1]) and bool(self._is_c_local[lvl][0]) and
                      (rank == 0 or bool(self.first_is_f_point[lvl])) and (rank == size - 1 or bool(self.last_is_c_point[lvl])))
        return all(self.comm_time.allgather_object(bool(ok)))

    def _one_rank_like(self) -> bool:
        """no exchange point falls INSIDE a whole-level pass: one rank, or ranks whose shares end on C-points (_detect_aligned)"""
        return self.comm_time_size == 1 or getattr(self, "_aligned", False)

    def _xpairs(self, lvl):
        """(fine slot, coarse slot) of the level's local C-points including the frozen one in front: the first point of the time
        grid on rank 0 (it is an owned C-point there), the ghost point (slot 0 on both levels) on an aligned rank > 0"""
        def build():
            own = self._pairs(lvl, skip_first=False)
            if self.comm_time_rank > 0 and getattr(self, "_aligned", False):
                return IndexArray(np.concatenate((np.zeros((1, 2), dtype=np.int64), as_index_array(own, 2))), width=2)
            return own
        return self._cached(('xpair', lvl), build)

    def _x0(self, lvl, send_row=None, staged=None):
        """op 0, the exchange point at the head of an F-relaxation (mgrit.py:304-311): the last local C-point to the next
        owner's ghost slot. send_row: the row that HOLDS that value when it is not the point's own row (pre-relaxed C-points);
        staged: the (fine, coarse) pair whose corrected value is sent before the pass that corrects it in place has run"""
        send = self._last_slot(lvl) if self.last_is_c_point[lvl] else None
        recv = 0 if self.first_is_f_point[lvl] else None
        if send is None and recv is None:
            return
        if staged is not None and send is not None:
            self.backend.exchange_staged(lvl, 0, staged, dest=self.send_to[lvl], recv_idx=recv, src=self.get_from[lvl])
        else:
            self.backend.exchange(lvl, 0, send_idx=(send_row if (send_row is not None and send is not None) else send),
                                  dest=self.send_to[lvl], recv_idx=recv, src=self.get_from[lvl], raw=True)

    def _x4(self, lvl):
        """op 4 of fas_residual(lvl) (mgrit.py:511-517): the last local point of lvl+1 to the next owner's ghost slot, then the
        clone of the received ghost into v (mgrit.py:520)"""
        up = lvl + 1
        send = int(self.index_local[up][-1]) if self.send_to[up] >= 0 else None
        recv = 0 if self.get_from[up] >= 0 else None
        if send is None and recv is None:
            return
        self.backend.exchange(up, 4, send_idx=send, dest=self.send_to[up], recv_idx=recv, src=self.get_from[up], raw=True)
        if recv is not None:
            self.backend.copy_pairs_u_to_v(lvl, self._cached(('pair_ghost_x', lvl), lambda: [(0, 0)]))

    def _head(self, lvl, head, which):
        """one rank: the first point of the time grid is relaxed and corrected by nobody, so its injection into level lvl+1
        (u, then the clone into v: mgrit.py:498-500, 520) writes the same row in every cycle -- two launches of a few microseconds
        that a small hierarchy notices. Done once, and again after anything has been written into the slabs from outside."""
        done = self.__dict__.setdefault('_head_done', set())
        gen = getattr(self.backend, "write_generation", lambda: None)()
        if gen is None:
            done.clear()
        elif gen != self.__dict__.get('_head_gen'):
            done.clear()
            self._head_gen = gen
        if (lvl, which) in done:
            return
        if which == 'u':
            self.backend.restrict_u(lvl, head)
            for key in [k for k in done if k[0] > lvl or k == (lvl, 'v')]:   # the levels below copy from the row just written (nested
                done.discard(key)                                           # iteration reaches them before level 0 has injected)
        else:
            self.backend.copy_pairs_u_to_v(lvl, head)
        if gen is not None:      # (while a cycle is being recorded: the recorded cycle runs right away and does it; the cycles
            done.add((lvl, which))   # recorded after it leave it out; _planned keys its plans by the write generation)

    def _x0_relaxed(self, lvl, pre=False):
        """aligned ranks: op 0 of the F-relaxation inside a whole-level down pass (mgrit.py:306-310) wants the RELAXED last
        C-point, which the pass itself computes. pre (pre-relaxed C-points, backend_hip._f_stale == 2): the cycle before has left
        exactly that value in the row of the last F-point; otherwise it is computed up front by a C-relaxation of that one point
        (the pass recomputes the same bits from the same F-point)"""
        last = self._last_slot(lvl)
        if pre:
            self._x0(lvl, send_row=last - 1)
            return
        if self.last_is_c_point[lvl]:
            self.backend.relax(lvl, self._cached(('c_last', lvl), lambda: [(last, 1)]), 'C')
        self._x0(lvl)

    def _last_pair(self, lvl):
        """the last local C-point as a one-pair list (aligned ranks: the row ops 0 / 4 send ahead of the pass that writes it)"""
        return self._cached(('pair_last', lvl), lambda: [self._xpairs(lvl)[-1]])

    def _up(self, lvl, fused, gen=None):
        """error correction + F-relaxation of level lvl on the way up (mgrit.py:283-284), in the most fused form available.
        gen: the way down of this cycle was mgrit_hip_gen_down over the same intervals"""
        res = lvl == 0 and self.conv_crit in (0, 2)     # the pass also leaves the residual check's sums
        shard = self._rank_intervals_up(lvl) if (gen is None and fused is None and lvl == 0 and self.comm_time_size > 1) else None
        if shard is not None:
            # several ranks: correction + F-relaxation + residual sums of the rank's complete intervals in one pass; the first
            # local C-point is corrected up front (the interval it closes belongs to the rank before), the partial intervals at
            # the two ends follow as plain F-relaxations with their exchange points; the residual of the first local C-point is
            # the residual kernel's (it needs the ghost point of op 7)
            intervals, c0_pair, edge_runs, n_head = shard
            buf = self.backend.residual_reserve(self._c_points(0), n_head)
            self.backend.error_correction(lvl, c0_pair)
            self.backend.ec_relax_res_to(lvl, intervals, buf)
            self.f_relax(lvl=lvl, runs=edge_runs)
            return
        whole = None
        if gen is None:     # level 0: the down pass's intervals; a coarser level: the same pass with g, no residual
            whole = fused if (fused is not None and res) else self._level_intervals(lvl, up=True) if lvl > 0 else None
        if gen is not None or whole is not None:
            if self.comm_time_size > 1:     # aligned ranks: op 0 of the F-relaxation (mgrit.py:306-310) carries the CORRECTED last
                self._x0(lvl, staged=self._last_pair(lvl))      # C-point, which the pass corrects in place only later
            if gen is not None:
                self.backend.gen_up(lvl, gen, residual=res)
            else:
                self.backend.ec_relax_res(lvl, whole)
            if res:
                self.backend.residual_ready(self._c_points(0))
        elif self._can_fuse_ec(lvl):
            self._ec_f_relax(lvl)
        else:
            self.error_correction(lvl=lvl)
            self.f_relax(lvl=lvl)

    def _rank_share(self, lvl):
        """several ranks: (pairs, inner, edge, first_relaxed) when the rank's share of the level is complete intervals -- both
        C-points local, at least one F-point between them -- behind its first local C-point, plus at most two edge runs (the
        partial intervals it shares with its neighbours), else None. pairs: (fine slot, coarse slot) of every local C-point;
        inner: the F-run of every complete interval; first_relaxed: False on rank 0 (global point 0)"""
        pairs = list(self._pairs(lvl, skip_first=False))
        if len(pairs) < 3:
            return None
        c0, ck = pairs[0][0], pairs[-1][0]
        runs = [tuple(r) for r in self._f_runs(lvl)]
        inner = [(pairs[k][0] + 1, pairs[k + 1][0] - pairs[k][0] - 1) for k in range(len(pairs) - 1)]
        edge = [r for r in runs if r[0] < c0 or r[0] > ck]
        relaxed = set(self._c_points(lvl))
        first_relaxed = c0 in relaxed
        if (any(ln < 1 for _, ln in inner) or sorted(inner + edge) != sorted(runs) or len(edge) > 2 or
                any(p[0] not in relaxed for p in pairs[1:]) or (first_relaxed and c0 < 1)):
            return None
        return pairs, inner, edge, first_relaxed

    def _rank_intervals_up(self, lvl):
        """several ranks, level 0, residual criterion: (intervals, c0_pair, edge_runs, n_head) for the way up on the rank's complete
        intervals (mgrit_hip_ec_relax_res_to), else None. res_pos of an interval = position of its closing C-point among the
        rank's relaxed C-points (the order of the residual values); n_head = how many of those lie in front of the first closing
        point (1: the first local C-point on ranks > 0; 0 on rank 0)."""
        def build():
            down = self._rank_intervals(lvl)
            if (down is None or self.conv_crit != 0 or
                    not self._can_fuse_ec(lvl) or getattr(self.backend, "residual_reserve", None) is None):
                return None
            ivals, c0_run, edge = (list(x) for x in down)
            cpts = list(self._c_points(lvl))
            pos = {c: i for i, c in enumerate(cpts)}
            if any(iv[1] not in pos for iv in ivals):
                return None
            n_head = pos[ivals[0][1]]
            if n_head != len(c0_run) or [pos[iv[1]] for iv in ivals] != list(range(n_head, n_head + len(ivals))) or \
                    n_head + len(ivals) != len(cpts):
                return None
            up = [(cs, ce, jcs, jce, pos[ce], keep) for (cs, ce, jcs, jce, _, keep) in ivals]
            corrected = dict(self._pairs(lvl, skip_first=True))
            c0_pair = [(c0_run[0][0], corrected[c0_run[0][0]])] if c0_run else []
            return up, c0_pair, edge, n_head
        return self._cached(('rank_intervals_up', lvl), build)

    def _coarse_down_rank(self, lvl):
        """several ranks, a level > 0 the finer level's FAS sweep has just filled: (fc_runs, c0_run, edge_runs) when the rank's
        complete intervals can take the two coarse-level passes (relax mode FC, fas_fused with_f_relax), else None"""
        def build():
            can = getattr(self.backend, "can_fuse_coarse_down", None)
            if not (not options.no_rank_fusion and self._own('coarse_down_rank') and 0 < lvl < self.lvl_max - 1 and
                    self.weight_c == 1.0 and self.cf_iter[lvl] == 1 and self.global_conv_crit and
                    not getattr(self, "_sweep_timing", False) and can is not None and can(lvl)):
                return None
            share = self._rank_share(lvl)
            if share is None:
                return None
            pairs, inner, edge, first_relaxed = share
            return [(st, ln + 1) for st, ln in inner], [(pairs[0][0], 1)] if first_relaxed else [], edge
        return self._cached(('coarse_down_rank', lvl), build)

    def _rank_intervals(self, lvl):
        """several ranks, level 0: (intervals, c0_run, edge_runs) when the rank's complete intervals -- both C-points local -- can
        take the down pass mgrit_hip_cf_fas, else None. intervals: as _level_intervals (every coarse row kept: the exchanges and
        the generic sweeps of the coarser level read them); c0_run: the first local C-point as a run list for the generic
        C-relaxation (empty on rank 0, whose first point is never relaxed); edge_runs: the F-runs in front of the first and behind
        the last local C-point (the partial intervals this rank shares with its neighbours)."""
        def build():
            be = self.backend
            can = getattr(be, "can_fuse_level", None)
            if not (not options.no_rank_fusion and self._own('rank_intervals') and lvl == 0 and self.lvl_max > 1 and
                    self.weight_c == 1.0 and self.global_conv_crit and not getattr(self, "_sweep_timing", False) and
                    can is not None and can(lvl) and getattr(be, "can_fuse_fas", lambda l: False)(lvl)):
                return None
            share = self._rank_share(lvl)
            if share is None:
                return None
            pairs, _, edge, first_relaxed = share
            ivals = [(pairs[k][0], pairs[k + 1][0], pairs[k][1] if (k >= 1 or first_relaxed) else -1, pairs[k + 1][1], k, 3)
                     for k in range(len(pairs) - 1)]
            return ivals, [(pairs[0][0], 1)] if first_relaxed else [], edge
        return self._cached(('rank_intervals', lvl), build)

    def _whole_intervals(self, lvl, closing_relaxed=True):
        """one rank, or a rank whose share looks like one (_detect_aligned): (P, runs) when the level is whole intervals -- slot 0
        in front, then one run of at least one F-point between every two consecutive C-points --, else None. P: the [N, 2] array
        of _xpairs, runs: the [N - 1, 2] array of those F-runs. closing_relaxed: the C-points that close the intervals are exactly
        the level's relaxed C-points (the passes that relax or correct them per interval ask for it). Compared as arrays: 16384
        intervals at config 3."""
        P, R = as_index_array(self._xpairs(lvl), 2), as_index_array(self._f_runs(lvl), 2)
        if P.shape[0] < 2 or P[0, 0] != 0:
            return None
        if closing_relaxed and not np.array_equal(as_index_array(self._c_points(lvl), 1)[:, 0], P[1:, 0]):
            return None
        runs = np.stack((P[:-1, 0] + 1, P[1:, 0] - P[:-1, 0] - 1), axis=1)
        if R.shape != runs.shape or not np.array_equal(R, runs) or (runs[:, 1] < 1).any():
            return None
        return P, runs

    @staticmethod
    def _interval_rows(P, keep):
        """[(cstart, cend, cstart_coarse, cend_coarse, res_pos, keep)] of the intervals between the pairs P; nothing of the
        coarse level stands in front of the first interval (-1)"""
        jcs = P[:-1, 1].copy()
        jcs[0] = -1
        n_iv = P.shape[0] - 1
        return IndexArray(np.column_stack((P[:-1, 0], P[1:, 0], jcs, P[1:, 1], np.arange(n_iv), keep)), width=6)

    def _coarse_down(self, lvl):
        """(fc_runs, triples, head, skip_coarse_u) when the way down of level lvl > 0 can run as two passes (relax mode FC,
        fas_fused with_f_relax; backend_hip.can_fuse_coarse_down), else None: one rank, the library's own sweeps, weight 1,
        cf_iter 0 or 1, every F-point between two local C-points."""
        def build():
            can = getattr(self.backend, "can_fuse_coarse_down", None)
            if not (self._own('coarse_down') and self._one_rank_like() and self.weight_c == 1.0 and 0 < lvl < self.lvl_max - 1 and
                    self.cf_iter[lvl] in (0, 1) and not getattr(self, "_sweep_timing", False) and can is not None and can(lvl)):
                return None
            whole = self._whole_intervals(lvl, closing_relaxed=False)      # (its two passes go by runs and triples)
            if whole is None:
                return None
            P, runs = whole
            fc_runs = IndexArray(runs + np.array([0, 1]), width=2)             # the F-points and the C-point closing them
            triples = IndexArray(np.column_stack((P[1:, 0], P[:-1, 0], P[1:, 1])), width=3)
            skip_u = lvl + 1 == self.lvl_max - 1 and self._coarsest_u_unread()
            return fc_runs, triples, self._xpairs(lvl)[:1] if self.comm_time_rank == 0 else [], skip_u
        return self._cached(('coarse_down', lvl), build)

    def _level_intervals(self, lvl, up=False):
        """[(cstart, cend, cstart_coarse, cend_coarse, res_pos, keep)] of level lvl when its sweeps can run as whole-level passes
        (mgrit_hip_cf_fas / mgrit_hip_ec_relax_res), else None: one rank (no exchange point inside the pass), the library's own
        sweeps, weight 1, and a level whose F-points all lie between two local C-points."""
        def build():
            # up: the pass of the way up alone (error correction + F-relaxation), which exists for every level pair
            can = getattr(self.backend, "can_fuse_level_up" if up else "can_fuse_level", None)
            if not (self._own('level_intervals') and self._one_rank_like() and self.weight_c == 1.0 and lvl < self.lvl_max - 1 and
                    not getattr(self, "_sweep_timing", False) and     # per-sweep debug lines: sweep by sweep
                    can is not None and can(lvl) and (not up or self._can_fuse_ec(lvl))):
                return None
            whole = self._whole_intervals(lvl)
            if whole is None:
                return None
            # rows of lvl+1 that the down pass must really store for the closing C-point (include/mgrit_hip.h, keep): u only
            # where the coarse level reads it before writing it -- its C-points when it starts with an F-relaxation (always,
            # mgrit.py:270-271), nothing on a coarsest level that forward_solve overwrites from its first point on --, v only
            # when the correction on the way up is not the pass that takes v from the fine C-point
            coarsest = lvl + 1 == self.lvl_max - 1
            jce = whole[0][1:, 1]                            # coarse slot of the C-point an interval ends on
            c_next = np.asarray(self.index_local_c[lvl + 1], dtype=np.int64)
            need_u = np.full(jce.size, not self._coarsest_u_unread()) if coarsest else np.isin(jce, c_next)
            need_v = 0 if (lvl == 0 and self.conv_crit in (0, 2)) else 2
            # ... and where the coarse level's first pass (relax mode FC, _coarse_down) starts its runs from v: its C-points
            v_start = np.isin(jce, c_next) if (not coarsest and self._coarse_down(lvl + 1) is not None) else np.zeros(jce.size, dtype=bool)
            keep = need_u.astype(np.int64) | need_v | (2 * v_start.astype(np.int64))
            # aligned ranks: the last local point travels to the next owner (op 4: u^{l+1}) and its corrected value is staged for
            # op 0 of the way up from u^{l+1} and v^{l+1} (Mgrit._x0): both rows are kept there
            if self.comm_time_size > 1 and self.send_to[lvl + 1] >= 0:
                keep[-1] |= 3
            return self._interval_rows(whole[0], keep)
        return self._cached(('intervals', lvl, up), build)

    def _gen_intervals(self, lvl):
        """[(cstart, cend, cstart_coarse, cend_coarse, res_pos, 3)] of level lvl when its sweeps can run as the general
        whole-level passes (mgrit_hip_gen_down / mgrit_hip_gen_up: any 1-D stepper pair, any of the library's transfers), else
        None: one rank, the library's own sweeps, weight 1, every F-point between two local C-points."""
        def build():
            can = getattr(self.backend, "can_gen_level", None)
            if not (self._own('gen_intervals') and self._one_rank_like() and self.weight_c == 1.0 and lvl < self.lvl_max - 1 and
                    self._dry is None and not getattr(self, "_sweep_timing", False) and can is not None and can(lvl)):
                return None
            whole = self._whole_intervals(lvl)
            return None if whole is None else self._interval_rows(whole[0], np.full(whole[0].shape[0] - 1, 3))
        return self._cached(('gen_intervals', lvl), build)

    def _can_fuse_ec(self, lvl):
        return (getattr(self.backend, "can_fuse_ec", None) is not None and self.backend.can_fuse_ec(lvl) and
                self._own('fuse_ec'))
