"""Pure-Python SRS v1-F: SRS v1 with crashed nodes and lost messages.

TEST INFRASTRUCTURE: the one definition of the failure semantics outside the kernels
(gp_ensemble_faults.hip); tests compare the GPU with it bit for bit, and
tools/failure_curves.py --backend ref runs its sweep through it.  A literal mirror of
oracle/srs_py.py's PySim; everything not marked "v1-F" is SRS v1 unchanged.
Loops are pure Python: keep P below ~1e3 and the rounds in the hundreds.
"""
from __future__ import annotations

import math

from oracle.srs_py import (STREAM_GOSSIP, STREAM_INJECT, STREAM_PUSHSUM, STREAM_START, build_neighbours,
                           philox4x32_10, resolve, uniform)

STREAM_FAULT_NODE, STREAM_FAULT_DROP = 5, 6
MASK = 0xFFFFFFFF
CONVERGED, MAX_ROUNDS, RUNNING = 0, 1, 2  # GP_STATUS_*
DOWN = 0x10  # flag bit 4


def threshold(p):
    """q = floor(p * 2**32) (exact in double); an event happens iff x < q."""
    if not (0.0 <= p <= 1.0):
        raise ValueError(p)
    return int(math.floor(p * 4294967296.0))


def ratio(s, w):
    """s / w as IEEE double division has it (a node that sent into the void for a thousand
    rounds has halved its weight down to 0)."""
    if w != 0.0:
        return s / w
    return float("nan") if s == 0.0 or s != s else math.copysign(float("inf"), s)


def draw_x(seed, stream, node, rnd):
    """First output word of the Philox call with counter (node, round, stream)."""
    return philox4x32_10((node & MASK, rnd, stream, node >> 32), (seed & MASK, seed >> 32))[0]


class FaultSim:
    """Literal synchronous-round simulator with the failure model (SRS v1-F)."""

    def __init__(self, num_nodes, topology, algorithm, seed=1, node_fail=0.0, msg_drop=0.0, fail_round=0,
                 max_rounds=400):
        if fail_round < 0:
            raise ValueError(fail_round)
        self.topology, self.algorithm, self.seed = topology, algorithm, seed
        self.P, self.T, self.g = resolve(num_nodes, topology)
        self.nbrs, self.nlat = build_neighbours(self.P, self.g, topology, seed)
        self.seed_node = uniform(seed, STREAM_START, 0, 0, self.T)
        self.round = 0
        self.alerts_total = 0  # counted alerts: nodes outside D only
        self.alerts = []       # per round
        self.max_rounds = max_rounds
        # v1-F: the doomed set, fixed at setup; the seed node never fails
        self.q_node, self.q_drop, self.fail_round = threshold(node_fail), threshold(msg_drop), fail_round
        self.D = [i != self.seed_node and draw_x(seed, STREAM_FAULT_NODE, i, 0) < self.q_node for i in range(self.P)]
        self.doomed = sum(self.D)
        self.threshold = max(1, self.T - self.doomed)
        self.lost = 0
        if algorithm == "gossip":
            self.c = [0] * self.P
            self.live = list(range(self.T)) if topology != "full" else None
        else:
            self.s = [float(i) for i in range(self.P)]
            self.w = [1.0] * self.P
            self.cnt = [1] * self.P
            self.conv = [False] * self.P
            self.active = [False] * self.P
            self.active[self.seed_node] = True

    # -- v1-F helpers -------------------------------------------------------
    def is_down(self, i, r):
        return self.D[i] and r >= self.fail_round

    def _dropped(self, i, r):
        """The sender's drop draw; none is made when q_drop == 0."""
        return self.q_drop > 0 and draw_x(self.seed, STREAM_FAULT_DROP, i, r) < self.q_drop

    @property
    def down(self):
        return self.doomed if self.round >= self.fail_round else 0

    @property
    def done(self):
        return self.alerts_total >= self.threshold or self.round >= self.max_rounds

    @property
    def status(self):
        if self.alerts_total >= self.threshold:
            return CONVERGED
        return MAX_ROUNDS if self.round >= self.max_rounds else RUNNING

    # -- gossip -------------------------------------------------------------
    def _gossip_round(self):
        r = self.round
        conv = [ci >= 11 for ci in self.c]
        inc = [0] * self.P
        for i in range(self.P):
            ci = self.c[i]
            if not ((i == self.seed_node or ci >= 1) and ci <= 10):
                continue
            if self.is_down(i, r):  # v1-F: a down node is not active
                continue
            t = self.nbrs[i][uniform(self.seed, STREAM_GOSSIP, i, r, len(self.nbrs[i]))]
            if self._dropped(i, r):  # v1-F
                self.lost += 1
            elif self.is_down(t, r):  # v1-F
                self.lost += 1
            elif not conv[t]:
                inc[t] += 1
        if self.live is not None and len(self.live) > 0:
            k = uniform(self.seed, STREAM_INJECT, 0, r, len(self.live))
            t = self.live[k]
            if conv[t] or self.is_down(t, r):  # v1-F: a down node is treated like a converged one
                self.live.remove(t)
            else:
                inc[t] += 1  # (the injector's messages are never dropped)
        alerts = 0
        for j in range(self.P):
            if inc[j]:
                if self.c[j] <= 10 < self.c[j] + inc[j] and not self.D[j]:  # v1-F: only nodes outside D count
                    alerts += 1
                self.c[j] += inc[j]
        return alerts

    # -- push-sum -----------------------------------------------------------
    def _pushsum_round(self):
        r = self.round
        inbox = [[] for _ in range(self.P)]
        msg = {}
        sends = [self.active[i] and not self.is_down(i, r) for i in range(self.P)]  # v1-F
        for i in range(self.P):
            if not sends[i]:
                continue
            k = uniform(self.seed, STREAM_PUSHSUM, i, r, len(self.nbrs[i]))
            t = self.nbrs[i][k]
            if self._dropped(i, r) or self.is_down(t, r):  # v1-F: the sent half leaves the network
                self.lost += 1
                continue
            msg[i] = (self.s[i] * 0.5, self.w[i] * 0.5)
            inbox[t].append((i, k < self.nlat[i]))
        alerts = 0
        news, neww = list(self.s), list(self.w)
        for j in range(self.P):
            if self.is_down(j, r):  # v1-F: frozen
                assert not inbox[j]
                continue
            s0, w0 = self.s[j], self.w[j]
            acc_s = s0 * 0.5 if sends[j] else s0
            acc_w = w0 * 0.5 if sends[j] else w0
            if inbox[j]:
                lattice = [snd for snd, lat in inbox[j] if lat]
                rand = sorted(snd for snd, lat in inbox[j] if not lat)
                ordered = [n for n in self.nbrs[j][: self.nlat[j]] if n in lattice] + rand
                assert len(ordered) == len(inbox[j])
                for snd in ordered:
                    acc_s = acc_s + msg[snd][0]
                    acc_w = acc_w + msg[snd][1]
                if not self.conv[j]:
                    self.cnt[j] = 0 if abs(ratio(acc_s, acc_w) - ratio(s0, w0)) > 1e-10 else self.cnt[j] + 1
                    if self.cnt[j] == 3:
                        self.conv[j] = True
                        if not self.D[j]:  # v1-F: only nodes outside D count
                            alerts += 1
                self.active[j] = True
            news[j], neww[j] = acc_s, acc_w
        self.s, self.w = news, neww
        return alerts

    def step(self, nrounds):
        """Up to nrounds rounds; stops after the round in which the counted alerts reach T_f, or
        at max_rounds.  Returns the per-round counted alerts of the rounds run."""
        out = []
        while len(out) < nrounds and not self.done:
            a = self._gossip_round() if self.algorithm == "gossip" else self._pushsum_round()
            out.append(a)
            self.alerts_total += a
            self.round += 1
        self.alerts += out
        return out

    def run(self):
        self.step(self.max_rounds)
        return self

    def flags(self):
        """The gp_ensemble_read_state byte: bit0 active, bit1 converged, bits2-3 count, bit4 down
        at the current round count.  A down gossip node is not active; a down push-sum node keeps
        the active bit it had."""
        dn = [DOWN if self.is_down(i, self.round) else 0 for i in range(self.P)]
        if self.algorithm == "gossip":
            return [(int((i == self.seed_node or ci >= 1) and ci <= 10 and not dn[i]) | (int(ci >= 11) << 1) | dn[i])
                    for i, ci in enumerate(self.c)]
        return [int(a) | (int(cv) << 1) | (cn << 2) | d for a, cv, cn, d in zip(self.active, self.conv, self.cnt, dn)]

    def stats(self):
        """(doomed, down, threshold, lost): the gp_fault_stats record."""
        return self.doomed, self.down, self.threshold, self.lost
