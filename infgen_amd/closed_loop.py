"""Closed-loop stepping sessions: a planner, a policy or a rule-based controller commands some rows of a rollout one
decode step at a time, from what the other agents did so far, while the model generates everyone else.

    ses = engine.RolloutEngine(..., replay=[mask]).session(pose='token')      # or InfGenDecoder.closed_loop(data, controlled='ego')
    while not ses.done:
        obs = ses.observe()                          # device tensors of the newest stored column, no synchronisation
        ses.command(poses=controller(obs))           # or command(tokens=...); device tensors, [S, A_cap(, 3)] or ego-only [S(, 3)]
        ses.advance()                                # the command kernel + one decode step (+ the step's insertion sub-loop)
    out = ses.outputs()

The repository's own controller is ``ses.command_idm(routes=...)`` in place of ``command`` (``run_idm`` loops it to the end): the
controlled rows follow their routes under the intelligent-driver car-following law, computed on the device.

A session is log replay (``RolloutEngine(replay=...)``) whose plan is written column by column: ``advance`` launches
``infgen_command_rows``, which turns the step's commands into the plan entries of column 2 + t on the device - a token id as it is, a
target pose through the nearest motion token of the row's vocabulary - and then runs the decode step, whose ``k_integrate`` forces
those entries on the flagged rows.  Nothing is read back per step (with scenario insertion on, the reads of its sub-loop remain).
Sessions run eagerly: no HIP graph is captured or replayed for them.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import _lib, constraints, controllers, observe

KIND_TOKEN, KIND_POSE = 0, 1


class ClosedLoopSession:
    """one stepping pass over a ``RolloutEngine``'s batch; made by ``RolloutEngine.session`` / ``InfGenDecoder.closed_loop``.

    ``t``: the decode step the next ``advance`` runs; ``done``: every step has run; ``cost`` [S, A_cap]: the matching cost of the
    last pose command per row (sum of the four corner distances between the commanded box and the matched token's, metres)."""

    def __init__(self, eng, pose: str = 'token', controlled=None, finish=None):
        if pose not in ('token', 'exact'):
            raise ValueError(f"pose must be 'token' or 'exact', not {pose!r}")
        if eng.teacher_token is not None and eng.replay_row is None:
            raise ValueError('an engine built with teacher= forces every row from its plan: a session needs replay= or controlled=')
        if controlled is None and eng.replay_row is None:
            raise ValueError("no controlled rows: build the engine with replay=[mask] or pass controlled='ego' / a bool tensor")
        self.eng, self.pose, self._finish = eng, pose, finish
        S, A_cap, dev = eng.S, eng.A_cap, eng.device
        eng.prologue()                                  # (its reset() ends a session that was still open)
        eng._bc_host = None
        # the plan buffers: pointers of the context change only when this engine never had them (or had the other pose mode) - a
        # graph captured for rollout() comes back with the pointers it was captured with when the session ends
        had_rows = eng.replay_row is not None
        self._restore = (had_rows, eng.teacher_pos is not None, eng._graph, eng._wgraph,
                         eng.replay_row.clone() if had_rows and controlled is not None else None)
        eng._alloc_replay(pose == 'exact')
        if controlled is not None:
            eng.replay_row.copy_(self._rows(controlled, torch.uint8, 'controlled'))
        # only rows of the initial scene are controlled (rows scenario insertion appends are always generated)
        rows = torch.arange(A_cap, device=dev)
        eng.replay_row.mul_((rows[None, :] < eng.n_agents[:, None]).to(torch.uint8))
        hc = eng.hc
        eng.teacher_token[:, hc:].fill_(-1)             # the logged future is not the plan: "no token" until commanded
        eng.teacher_state[:, hc:].zero_()
        if eng._replay_pose is not None:
            for buf in eng._replay_pose:
                buf[:, hc:].zero_()
        self._tok = torch.zeros(S, A_cap, dtype=torch.int32, device=dev)
        self._pose = torch.zeros(S, A_cap, 3, device=dev)
        self._mask = torch.ones(S, A_cap, dtype=torch.uint8, device=dev)
        self.cost = torch.zeros(S, A_cap, device=dev)
        self._kind = self._result = None
        self._idm = None                                # command_idm()'s result buffers, allocated at its first call
        self._look = None                               # lookahead()'s snapshot buffer, allocated at its first call
        self._obs_rows, self._obs_out, self._obs_key = {}, None, None     # observe(frame='agent'): row lists, the last result
        self.t = 0
        self.steps = eng.cfg.num_decode_steps
        eng._refresh_opts(groups=True)
        eng._session = self

    # ------------------------------------------------------------------ state
    @property
    def done(self) -> bool:
        return self.t >= self.steps

    @property
    def open(self) -> bool:
        return self.eng._session is self

    def _check_open(self):
        if not self.open:
            raise RuntimeError('this session has ended (the engine was reset, reloaded or given a new session)')

    def _end(self):
        """called by the engine's ``reset``: the context's plan pointers go back to what a captured graph saw"""
        eng = self.eng
        eng._session = None
        had_rows, had_pose, graph, wgraph, flags = self._restore
        if had_rows:
            eng._alloc_replay(had_pose)
            eng._graph, eng._wgraph = graph, wgraph
            if flags is not None:
                eng.replay_row.copy_(flags)
        else:
            eng.replay_row.zero_()             # an engine that replayed nothing before the session generates every row again

    def _rows(self, x, dtype, what, tail=()):
        """[S, A_cap, ...] / [S, rows <= A_cap, ...] / ego-only [S, ...] / 'ego' -> a tensor of the full row layout (no host read)"""
        eng = self.eng
        S, A_cap, dev = eng.S, eng.A_cap, eng.device
        if isinstance(x, str):
            if x != 'ego':
                raise ValueError(f"{what} must be 'ego' or a tensor, not {x!r}")
            x = torch.ones(S, dtype=dtype, device=dev)
        x = torch.as_tensor(x).to(dev)
        if x.shape == (S,) + tuple(tail):                # one entry per scene: the ego's
            full = torch.zeros((S, A_cap) + tuple(tail), dtype=dtype, device=dev)
            full[torch.arange(S, device=dev), eng.av.long()] = x.to(dtype)
            return full
        if x.dim() == 2 + len(tail) and x.shape[0] == S and x.shape[1] <= A_cap and tuple(x.shape[2:]) == tuple(tail):
            if x.shape[1] == A_cap:
                return x.to(dtype)
            full = torch.zeros((S, A_cap) + tuple(tail), dtype=dtype, device=dev)
            full[:, :x.shape[1]] = x.to(dtype)
            return full
        raise ValueError(f'{what}: expected shape {(S, A_cap) + tuple(tail)} or {(S,) + tuple(tail)}, got {tuple(x.shape)}')

    # ------------------------------------------------------------------ the loop
    def observe(self, frame: str = 'world', rows='controlled', neighbors: int = 8, radius: float = float('inf'),
                map_tokens: int = 0, map_radius: float = float('inf')) -> Dict[str, torch.Tensor]:
        """the newest stored column as device tensors: ``pos`` [S, A_cap, 2], ``head``, ``state`` (0 = not in the scene), ``token``,
        ``type`` [S, A_cap], ``shape`` [S, A_cap, 3] (length, width, height), ``n_agents`` / ``ego_index`` [S], ``controlled``
        [S, A_cap] bool and ``column`` (int); with ``avoid_collisions`` also ``allowed_tokens`` [S, A_cap], the number of motion tokens
        every row was allowed at the step that just ran, before the empty-set fallback (0: every token collided); with ``stay_on_road`` the
        sizes of the final sets, the road masks' (0: every token of the row's collision or static set left the road).  Views of the engine's buffers wherever possible: no copy, no synchronisation - and
        overwritten by later steps, a reset or a reload (clone what has to last).

        ``frame='agent'`` adds the agent-centric observation of that column (``RolloutEngine.observe_rows``: one launch,
        no host read): ``obs_row`` [N] int32, the global rows s * A_cap + i observed, and per observed row ``self_feat`` [N, 8],
        the ``neighbors`` nearest live agents within ``radius`` - ``nbr_feat`` [N, K, 10], ``nbr_index`` [N, K], ``nbr_count`` [N] -
        and the ``map_tokens`` nearest map tokens within ``map_radius`` - ``map_feat`` [N, Km, 6], ``map_index``, ``map_count`` -, in
        the row's own frame.  ``rows``: 'controlled' (the rows this session commands, in row order), 'all' or an int tensor of global
        rows.  The list of controlled rows is built once per session, on the device, at the first such call - its length is the
        one host read, none per step.  The result's tensors are the session's own and are written again by the next call of the
        same sizes.  The arguments other than ``frame`` are read only with ``frame='agent'``."""
        self._check_open()
        if frame not in ('world', 'agent'):
            raise ValueError(f"frame must be 'world' or 'agent', not {frame!r}")
        eng, c = self.eng, self.eng.hc - 1 + self.t
        obs = dict(pos=eng.pos[:, c], head=eng.head[:, c], state=eng.state[:, c], token=eng.token[:, c], type=eng.atype,
                   shape=eng._shape10, n_agents=eng.n_agents, ego_index=eng.av, controlled=eng.replay_row.bool(), column=c)
        if eng.avoid_collisions is not None:      # collision-aware decoding: the sizes of the sets the last step decoded under
            obs['allowed_tokens'] = eng.collision_allowed.view(eng.S, eng.A_cap)
        if eng.stay_on_road is not None:          # road-aware decoding runs behind the collision masks
            obs['allowed_tokens'] = eng.road_allowed.view(eng.S, eng.A_cap)
        if eng.obey_signals is not None:          # signal-aware decoding runs behind the road masks; gap, line, flag, 0 per row
            obs['allowed_tokens'] = eng.signal_allowed.view(eng.S, eng.A_cap)
            obs['signal'] = eng.signal_info.view(eng.S, eng.A_cap, 4)
        if eng.follow_routes is not None:         # route-following decoding runs last: its sets are the ones the heads read
            obs['allowed_tokens'] = eng.route_allowed.view(eng.S, eng.A_cap)
            obs['route_progress'] = eng.route_progress.view(eng.S, eng.A_cap, 4)
        if eng.step_scores is not None:           # step scores: the step that just ran (absent before the first) and its rows' flags
            if self.t > 0:
                obs['step_score'] = eng.step_score[:, self.t - 1]
            obs['score_row'] = eng.score_row
        if self._idm is not None:                 # command_idm: what the last call found (s0, e0, v, gap, acc, v1, s1, flag; the lead)
            obs['idm_state'] = self._idm['state'].view(eng.S, eng.A_cap, 8)
            obs['idm_lead'] = self._idm['lead'].view(eng.S, eng.A_cap)
        if frame == 'agent':
            obs_row = self._observed_rows(rows)
            out = self._obs_out if self._obs_out is not None and self._obs_key == (int(obs_row.numel()), neighbors, map_tokens) else None
            self._obs_out = eng.observe_rows(c, rows=None if isinstance(rows, str) and rows == 'all' else obs_row, neighbors=neighbors,
                                             radius=radius, map_tokens=map_tokens, map_radius=map_radius, out=out)
            self._obs_key = (int(obs_row.numel()), neighbors, map_tokens)
            obs.update(self._obs_out, obs_row=obs_row)
        return obs

    def _observed_rows(self, rows) -> torch.Tensor:
        """'controlled' | 'all' | int tensor -> int32 [N] global rows on the device ('controlled' and 'all': made once per session)"""
        eng = self.eng
        if isinstance(rows, str):
            if rows not in ('controlled', 'all'):
                raise ValueError(f"rows must be 'controlled', 'all' or an int tensor, not {rows!r}")
            if rows not in self._obs_rows:
                self._obs_rows[rows] = (torch.nonzero(eng.replay_row.reshape(-1)).reshape(-1).to(torch.int32) if rows == 'controlled'
                                        else torch.arange(eng.S * eng.A_cap, device=eng.device, dtype=torch.int32))
            return self._obs_rows[rows]
        observe.check_rows(rows)
        return rows.to(eng.device, torch.int32).contiguous()

    def command(self, tokens=None, poses=None, mask=None):
        """the controlled rows' command for step ``t``: ``tokens`` (motion-token ids, int) or ``poses`` (x, y, heading in the world
        frame), as [S, A_cap] / [S, A_cap, 3] tensors (entries of uncontrolled rows are ignored) or [S] / [S, 3] for the ego alone;
        ``mask`` (same layouts, optional): False = the row leaves the scene at this step and stays out.  Device tensors are taken as
        they are (stream-ordered, no synchronisation); a later ``command`` before ``advance`` replaces this one."""
        self._check_open()
        if self.done:
            raise RuntimeError('the session has run its last step')
        if (tokens is None) == (poses is None):
            raise ValueError('give tokens= or poses=, one of them')
        if poses is not None and self.eng._shape10 is None:
            raise ValueError('a pose command needs the rows\' shapes: this engine has no shape array')
        if tokens is not None:
            self._tok.copy_(self._rows(tokens, torch.int32, 'tokens'))
            self._kind = KIND_TOKEN
        else:
            self._pose.copy_(self._rows(poses, torch.float32, 'poses', tail=(3,)))
            self._kind = KIND_POSE
        if mask is None:
            self._mask.fill_(1)
        else:
            self._mask.copy_(self._rows(mask, torch.uint8, 'mask'))

    def command_idm(self, routes=None, n_points=None, v_des=None, mask=None, **params):
        """the controlled rows' command for step ``t`` from the rule-based controller (``RolloutEngine.idm_command``):
        the session's pose buffer is filled with every row's current pose - a controlled row without a route, or of a type the
        rule does not cover, stands still -, ``infgen_idm_command`` writes the targets of the ruled rows over it from the newest
        stored column, and the pending command becomes that pose command.  ``routes`` / ``n_points``: the routes (None: the
        engine's ``follow_routes`` tables); ``v_des`` [S0][A]: own desired speeds; ``params``: the keys of
        ``controllers.check_idm``; ``mask`` as for ``command``.  Nothing is read on the host.  ``observe()['idm_state']``
        [S, A_cap, 8] = s0, e0, v, gap, acc, v1, s1, flag and ``['idm_lead']`` [S, A_cap] = j, -1, -2 show what it found."""
        self._check_open()
        if self.done:
            raise RuntimeError('the session has run its last step')
        eng, c = self.eng, self.eng.hc - 1 + self.t
        self._pose[..., :2].copy_(eng.pos[:, c])
        self._pose[..., 2].copy_(eng.head[:, c])
        if self._idm is None:
            self._idm = dict(controllers.idm_buffers(eng.S, eng.A_cap, eng.device), pose=self._pose)
        eng.idm_command(c, ctl_row=eng.replay_row, routes=routes, n_points=n_points, v_des=v_des, out=self._idm, **params)
        self._kind = KIND_POSE
        if mask is None:
            self._mask.fill_(1)
        else:
            self._mask.copy_(self._rows(mask, torch.uint8, 'mask'))

    def constrain(self, mask_row):
        """the rows' allowed-token sets from the next ``advance()`` on: ``mask_row`` [S, A_cap] (or [S, rows <= A_cap]) set indices
        into the engine's ``token_masks`` table, -1 = the row's type decides (the engine's ``token_mask_type``).  A device tensor is
        copied into the engine's static selector buffer as it is - stream-ordered, no host read, so a controller can tighten or
        release a row per step; an index beyond the table reads as unconstrained.  Rows the session controls keep their commands."""
        self._check_open()
        eng = self.eng
        if eng.token_masks is None:
            raise ValueError('constrain() needs an engine built with token_masks=')
        x = torch.as_tensor(mask_row)
        if x.is_floating_point() or x.dtype == torch.bool:
            raise ValueError('mask_row holds integer set indices')
        if not x.is_cuda:
            constraints.check_row_selectors(x.numpy(), eng.token_masks.n_sets)
        if x.dim() != 2 or x.shape[0] != eng.S or x.shape[1] > eng.A_cap:
            raise ValueError(f'mask_row: expected shape {(eng.S, eng.A_cap)}, got {tuple(x.shape)}')
        x = x.to(eng.device, torch.int32)
        if x.shape[1] < eng.A_cap:
            full = torch.full((eng.S, eng.A_cap), -1, dtype=torch.int32, device=eng.device)
            full[:, :x.shape[1]] = x
            x = full
        eng.mask_row.copy_(x.reshape(-1))

    def set_routes(self, routes, n_points):
        """new routes for the rows of an engine with ``follow_routes`` (``RolloutEngine.set_routes``): they rule from the next
        ``advance()`` on; ``observe()['route_progress']`` [S, A_cap, 4] = s0, d0, total, flag stays that of the step that just ran"""
        self._check_open()
        self.eng.set_routes(routes, n_points)

    def set_signals(self, phase=None, lines=None, n_lines=None):
        """new phase and / or stop-line tables for an engine with ``obey_signals`` (``RolloutEngine.set_signals``): they rule from
        the next ``advance()`` on - a planner's way to switch a light; ``observe()['signal']`` [S, A_cap, 4] = gap, line, flag, 0
        stays that of the step that just ran"""
        self._check_open()
        self.eng.set_signals(phase=phase, lines=lines, n_lines=n_lines)

    def branch(self, parent):
        """``RolloutEngine.branch(parent, t)`` at this session's step: slot s continues as a clone of slot ``parent[s]`` from the
        next ``advance()`` on - ``observe()`` then shows the parent's newest column in the child slot.  A pending
        command stays the slot's own, as do its controlled-row flags; past commands of the child are not read again.  The collision
        and road buffers are not cloned (every step rebuilds them from the poses): until the next ``advance()``,
        ``observe()['allowed_tokens']`` of a child slot still shows the sizes of the child's own sets of the step that just ran."""
        self._check_open()
        self.eng.branch(parent, self.t)

    # ------------------------------------------------------------------ snapshots
    def snapshot(self, slots=None, out=None):
        """``RolloutEngine.snapshot(t, ...)`` at this session's step: the decode state of every slot (or ``slots``) in front of the
        next ``advance()``, on the device.  The plan is not part of it: a restored slot follows the commands given after the
        restore."""
        self._check_open()
        return self.eng.snapshot(self.t, slots=slots, out=out)

    def restore(self, snap, index=None):
        """``RolloutEngine.restore(snap, index)``, and the session stands at step ``snap.t`` again: ``t = snap.t``, a pending command
        is dropped and the plan columns from that step on read "no token" again, as after ``__init__`` - the commands of the steps
        that are run again come from the caller.  ``observe()`` shows the restored newest column at once; the collision and road
        buffers are not part of a snapshot (every step rebuilds them), so ``observe()['allowed_tokens']`` stays that of the last
        step that ran - the look-ahead's, say - until the next ``advance()``."""
        self._check_open()
        eng = self.eng
        eng.restore(snap, index)
        self.t = int(snap.t)
        self._kind = None
        c = eng.hc + self.t
        eng.teacher_token[:, c:].fill_(-1)
        eng.teacher_state[:, c:].zero_()
        if eng._replay_pose is not None:
            for buf in eng._replay_pose:
                buf[:, c:].zero_()
        self._result = None

    def lookahead(self, horizon: int, tokens=None, poses=None, mask=None, weights=None) -> torch.Tensor:
        """try the given commands for ``H = min(horizon, steps - t)`` steps and come back: a snapshot of all slots into a buffer the
        session keeps, H x (``command``, ``advance``), ``branching.score_log_weight`` over the step scores of those steps, restore.
        ``tokens`` / ``poses`` / ``mask``: what ``command`` takes with a leading step axis, [>= H, ...]; ``weights``: a dict with
        keys of ``branching.SCORE_WEIGHTS``.  Returns the log weight [S0, copies] on the device (higher is better); nothing is read
        on the host.  With ``copies = K`` and one candidate plan per copy, ``argmax`` over the result gathered into the next
        ``command`` is one model-predictive-control step.  A command that was pending is pending again afterwards; ``cost`` is
        that of before the call.  Needs an engine built with ``step_scores``."""
        from . import branching
        self._check_open()
        eng = self.eng
        if eng.step_scores is None:
            raise ValueError('lookahead: needs step_scores (the engine logs no score to weigh the tries by)')
        if self.done:
            raise RuntimeError('the session has run its last step')
        if (tokens is None) == (poses is None):
            raise ValueError('give tokens= or poses=, one of them')
        if int(horizon) < 1:
            raise ValueError('lookahead: horizon must be at least 1')
        weights = branching.check_score_weights(weights)
        t0 = self.t
        H = min(int(horizon), self.steps - t0)
        cmd = tokens if tokens is not None else poses
        for what, x in (('commands', cmd), ('mask', mask)):
            if x is not None and (not isinstance(x, torch.Tensor) or x.dim() < 2 or x.shape[0] < H):
                raise ValueError(f'lookahead: {what} need a leading step axis of at least {H} entries')
        pending = None
        if self._kind is not None:
            pending = (self._kind, self._tok.clone(), self._pose.clone(), self._mask.clone())
        cost = self.cost.clone()
        if self._look is None:              # (a reload ends the session, so the layout cannot change under the buffer)
            self._look = eng.snapshot_buffer()
        snap = self.snapshot(out=self._look)
        for h in range(H):
            m = None if mask is None else mask[h]
            if tokens is not None:
                self.command(tokens=tokens[h], mask=m)
            else:
                self.command(poses=poses[h], mask=m)
            self.advance()
        lw = branching.score_log_weight(eng.step_score, t0, t0 + H, weights, copies=eng.copies)
        self.restore(snap)
        self.cost.copy_(cost)
        if pending is not None:
            self._kind = pending[0]
            self._tok.copy_(pending[1]); self._pose.copy_(pending[2]); self._mask.copy_(pending[3])
        return lw

    def advance(self):
        """the command kernel, then decode step ``t`` (with its insertion sub-loop when the engine inserts agents)"""
        self._check_open()
        if self.done:
            raise RuntimeError('the session has run its last step')
        if self._kind is None:
            raise RuntimeError(f'no command for step {self.t}: call command() before advance()')
        eng, P = self.eng, _lib.ptr
        _lib.check(eng.lib.infgen_command_rows(C.byref(eng._ctx), self.t, self._kind, P(self._tok), P(self._pose), P(self._mask),
                                               P(eng._shape10), P(self.cost), eng.ops.stream), 'infgen_command_rows')
        for _ in eng._step_gen(self.t):         # (the generator waits for each of the insertion sub-loop's events itself)
            pass
        self._kind = None
        self.t += 1

    # ------------------------------------------------------------------ results
    def _check_done(self):
        self._check_open()
        if not self.done:
            raise RuntimeError(f'the session is at step {self.t} of {self.steps}: outputs exist after the last step')

    def outputs(self):
        """after the last step: what the entry that made the session returns for a rollout - the engine's ``outputs()``, or the
        dict(s) of ``InfGenDecoder.inference`` for a session made by ``closed_loop``"""
        if self._result is None:
            self._check_done()
            self._result = self._finish() if self._finish is not None else self.eng.outputs()
        return self._result

    def outputs_device(self, detach: bool = False):
        self._check_done()
        return self.eng.outputs_device(detach=detach)

    def outputs_batch(self):
        self._check_done()
        return self.eng.outputs_batch()


def run_idm(session: ClosedLoopSession, **kw):
    """``command_idm(**kw)`` + ``advance()`` until the session's last step -> the session (``outputs()`` is ready)"""
    while not session.done:
        session.command_idm(**kw)
        session.advance()
    return session
