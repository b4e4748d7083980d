"""Rollout sink and metric features: mirror of the reference's formatting of close-loop rollouts
(infgen/model/infgen.py:788-835), `output_to_rollouts` (infgen/metrics/compute_metrics.py:360-463) and
`compute_metric_features` (:560-707).  The rollout arrays stay on the GPU from `InfGenDecoder.inference` to the features:
every feature is one launch of the HIP library (see the sibling modules); nothing is computed on the CPU.

Constants of the Waymo sim-agents submission spec the reference takes from `waymo_open_dataset` (a third-party package,
`submission_specs`): CURRENT_TIME_INDEX 10, STEP_DURATION_SECONDS 0.1; SHIFT 5 is the reference's token stride (:38).
"""
import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor

from . import interact_features, map_features, placement_features, trajectory_features

CURRENT_TIME_INDEX = 10
STEP_DURATION_SECONDS = 0.1
SHIFT = 5
AGENT_STATE = ['invalid', 'valid', 'enter', 'exit']
COLLISION_DISTANCE_THRESHOLD = 0.0


def get_scenario_id_int_tensor(scenario_id: List[str], device=torch.device('cpu')) -> Tensor:
    """reference compute_metrics.py:348-357: characters as int32, -1 padded to 16"""
    out = torch.full((len(scenario_id), 16), -1, dtype=torch.int32)
    for i, sid in enumerate(scenario_id):
        out[i, :len(sid)] = torch.tensor([ord(ch) for ch in sid], dtype=torch.int32)
    return out.to(device)


def format_rollouts(data, rollouts: Sequence[Dict[str, Tensor]], to_cpu: bool = False) -> Dict:
    """reference infgen.py:788-835: stack the per-rollout outputs of `InfGenDecoder.inference` on a new dim 1 into the dict
    that is pickled / handed to the metrics.  The reference moves every array to the CPU here; by default this keeps them
    where they are (`to_cpu=True` reproduces the pickled layout)."""
    keys = dict(pred_valid='pred_valid', token_pos='pos_a', token_head='head_a', pred_traj='pred_traj', pred_head='pred_head',
                pred_z='pred_z', pred_shape='eval_shape', pred_type='pred_type', pred_state='next_state_idx',
                agent_id='agent_id')
    out = {k: torch.stack([r[src] for r in rollouts], dim=1) for k, src in keys.items()}
    first = rollouts[0]
    if 'agent_batch' in first:
        # a multi-graph Batch decoded at once (InfGenDecoder.inference): rows of every graph concatenated, agent_batch per row,
        # ego_index [B] rows into the concatenation; av_id one per graph (a plain int for one graph, like the single-scene dict)
        ego = torch.as_tensor(first['ego_index']).reshape(-1).long()
        av = first['agent_id'][ego.to(first['agent_id'].device)].long()
        av_id = av if av.numel() > 1 else int(av[0])
        agent_batch = first['agent_batch'].long()
    else:
        av_id = int(first['agent_id'][int(first['ego_index'])])
        agent_batch = torch.zeros(out['pred_traj'].shape[0], dtype=torch.long, device=out['pred_traj'].device)
    out = dict(_scenario_id=data['scenario_id'], scenario_id=get_scenario_id_int_tensor(data['scenario_id']),
               av_id=av_id, agent_batch=agent_batch,
               tfrecord_path=data['tfrecord_path'] if 'tfrecord_path' in data else None, **out)
    if to_cpu:
        out = {k: v.cpu() if torch.is_tensor(v) else v for k, v in out.items()}
    return out


@dataclass(frozen=True)
class ObjectTrajectories:
    """reference compute_metrics.py:142-163 (fields and meaning)"""
    x: Tensor
    y: Tensor
    z: Tensor
    heading: Tensor
    length: Tensor
    width: Tensor
    height: Tensor
    valid: Tensor
    object_id: Tensor
    object_type: Tensor
    state: Optional[Tensor] = None
    token_pos: Optional[Tensor] = None
    token_heading: Optional[Tensor] = None
    token_valid: Optional[Tensor] = None
    processed_object_id: Optional[Tensor] = None
    av_id: Optional[int] = None
    processed_av_id: Optional[int] = None

    def gather_objects_by_id(self, object_ids: Tensor) -> 'ObjectTrajectories':
        """:187-213: rows of the given ids (10 Hz fields only; the token-rate fields stay whole, like the reference)"""
        hit = self.object_id[None, :] == object_ids.to(self.object_id.device)[:, None]
        if not bool(hit.any(1).all()):
            raise ValueError('Some items in `reference_tensor` are missing from `tensor`: '
                             f'\n{object_ids} \nvs. \n{self.object_id}.')
        idx = hit.int().argmax(1)
        rows = {f: getattr(self, f).index_select(-2, idx) for f in ('x', 'y', 'z', 'heading', 'length', 'width', 'height', 'valid')}
        return dataclasses.replace(self, object_id=self.object_id[idx], object_type=self.object_type[idx], **rows)


@dataclass(frozen=True)
class ScenarioRollouts:
    joint_scenes: List[ObjectTrajectories]
    scenario_id: str


def output_to_rollouts(scenario: Dict) -> List[ScenarioRollouts]:
    """reference compute_metrics.py:360-463: the rollouts dict -> per scenario, per rollout trajectories with the shape
    broadcast over the steps.  `object_type` is (n_agent,) here (the reference's repeat of a 2-D tensor yields an
    unusable shape, and no feature reads it)."""
    sid = scenario['scenario_id'].cpu()
    batch = scenario['agent_batch']
    n_scen = sid.shape[0]
    n_step = scenario['pred_traj'].shape[2]
    state = scenario['pred_state'] if 'pred_state' in scenario else torch.zeros_like(scenario['pred_z']).long()
    av_all = scenario.get('av_id', -1)
    out = []
    for s in range(n_scen):
        # av_id: one int for the scenario, or one per scenario of a batched dict
        av_s = int(av_all[s]) if torch.is_tensor(av_all) and av_all.numel() > 1 else av_all
        rows = torch.nonzero(batch == s)[:, 0]
        g = lambda k: scenario[k].index_select(0, rows)
        traj, shape, ids = g('pred_traj'), g('pred_shape'), g('agent_id')
        st = state.index_select(0, rows)
        scenes = []
        for r in range(traj.shape[1]):
            sh = shape[:, r, None, :].expand(-1, n_step, -1)
            scenes.append(ObjectTrajectories(
                x=traj[:, r, :, 0], y=traj[:, r, :, 1], z=g('pred_z')[:, r], heading=g('pred_head')[:, r],
                length=sh[..., 0], width=sh[..., 1], height=sh[..., 2], valid=g('pred_valid')[:, r], state=st[:, r],
                object_id=ids[:, r], processed_object_id=ids[:, r], object_type=g('pred_type')[:, r],
                token_pos=g('token_pos')[:, r, :, :2], token_heading=g('token_head')[:, r],
                av_id=av_s, processed_av_id=av_s))
        out.append(ScenarioRollouts(joint_scenes=scenes, scenario_id=''.join(chr(c) for c in sid[s].tolist() if c > 0)))
    return out


@dataclass(frozen=True)
class MetricFeatures:
    """reference compute_metrics.py:500-516"""
    object_id: Tensor
    valid: Tensor
    linear_speed: Tensor
    linear_acceleration: Tensor
    angular_speed: Tensor
    angular_acceleration: Tensor
    distance_to_nearest_object: Tensor
    collision_per_step: Tensor
    time_to_collision: Tensor
    distance_to_road_edge: Optional[Tensor]
    offroad_per_step: Optional[Tensor]
    num_placement: Tensor
    num_removement: Tensor
    distance_placement: Tensor
    distance_removement: Tensor


def compute_metric_features(simulate_trajectories: ObjectTrajectories, evaluate_agent_ids: Optional[Tensor] = None,
                            scenario_log=None, road_edge_polylines=None) -> MetricFeatures:
    """reference compute_metrics.py:560-707.  Road edges come from `scenario_log.map_features[*].road_edge.polyline`
    like there, or directly as `road_edge_polylines` (a list of polylines or the (padded, cyclic) pair of
    `map_features.tensorize_polylines`).  Without either the two map features are None (the reference leaves them
    uninitialised)."""
    sim = simulate_trajectories
    ev = sim.gather_objects_by_id(evaluate_agent_ids) if evaluate_agent_ids is not None else sim
    cut = CURRENT_TIME_INDEX + 1
    kin = trajectory_features.compute_kinematic_features(ev.x, ev.y, ev.z, ev.heading, seconds_per_step=STEP_DURATION_SECONDS)
    speed, accel, yaw_rate, yaw_accel = (k[:, cut:] for k in kin)
    every = torch.ones(sim.object_id.shape[0], dtype=torch.bool, device=sim.x.device)
    boxes = dict(center_x=sim.x, center_y=sim.y, length=sim.length, width=sim.width, heading=sim.heading, valid=sim.valid,
                 evaluated_object_mask=every)
    dist = interact_features.compute_distance_to_nearest_object(center_z=sim.z, height=sim.height, **boxes)[:, cut:]
    ttc = interact_features.compute_time_to_collision_with_object_in_front(seconds_per_step=STEP_DURATION_SECONDS,
                                                                           **boxes)[:, cut:]
    if road_edge_polylines is None and scenario_log is not None:
        road_edge_polylines = [f.road_edge.polyline for f in scenario_log.map_features if f.HasField('road_edge')]
    road = offroad = None
    if road_edge_polylines is not None:
        road = map_features.compute_distance_to_road_edge(center_z=sim.z, height=sim.height,
                                                          road_edge_polylines=road_edge_polylines, **boxes)[:, cut:]
        offroad = road > map_features.OFFROAD_DISTANCE_THRESHOLD
    if sim.av_id == sim.processed_av_id == -1:
        n_agent, n10 = speed.shape
        z1 = torch.zeros(n10 // SHIFT, device=sim.x.device)
        num_in, num_out = z1, z1.clone()
        d_in = torch.zeros(n_agent, n10 // SHIFT, device=sim.x.device)
        d_out = d_in.clone()
    else:
        assert sim.av_id == sim.processed_av_id, f'Got duplicated av_id: {sim.av_id} and {sim.processed_av_id}'
        c2 = CURRENT_TIME_INDEX // SHIFT
        num_in, num_out = (n[c2:] for n in placement_features.compute_num_placement(
            state=sim.state, valid=sim.token_valid, av_id=sim.processed_av_id, object_id=sim.processed_object_id,
            agent_state=AGENT_STATE))
        d_in, d_out = (d[:, c2:] for d in placement_features.compute_distance_placement(
            position=sim.token_pos, state=sim.state, valid=sim.valid, av_id=sim.processed_av_id,
            object_id=sim.processed_object_id, agent_state=AGENT_STATE))
    return MetricFeatures(object_id=sim.object_id, valid=ev.valid[:, cut:], linear_speed=speed, linear_acceleration=accel,
                          angular_speed=yaw_rate, angular_acceleration=yaw_accel, distance_to_nearest_object=dist,
                          collision_per_step=dist < COLLISION_DISTANCE_THRESHOLD, time_to_collision=ttc,
                          distance_to_road_edge=road, offroad_per_step=offroad, num_placement=num_in[None],
                          num_removement=num_out[None], distance_placement=d_in, distance_removement=d_out)


def to_host(t: Tensor) -> Tensor:
    """THE device -> host copy of the batched sink (`compute_metric_features_batch`, `scores.compute_scenario_metrics_batch`,
    `LongMetric.update_rollouts`): every value those read back goes through here, so a caller (or a test) can count them"""
    return t.cpu()


@dataclass(frozen=True)
class MetricFeaturesBatch:
    """`MetricFeatures` of every rollout of every scenario of a rollouts dict: the same fields with a leading B =
    n_scenario * n_rollout (bundle b = scenario * n_rollout + rollout), objects padded to N_max rows.  Padding rows are invalid,
    in state `invalid`, and no score reads them: `n_rows` [B] (device, int32) holds the real row count of every bundle - its
    scenario's, or fewer where a rollout lacks rows the scenario's other rollouts have (`align_rollouts`) -, `bundle` [B] the
    scenario a bundle belongs to.  The per-step fields are views that skip the history steps."""
    object_id: Tensor                    # [B][N], -1 on padding rows
    valid: Tensor                        # [B][N][T] bool
    linear_speed: Tensor
    linear_acceleration: Tensor
    angular_speed: Tensor
    angular_acceleration: Tensor
    distance_to_nearest_object: Tensor
    collision_per_step: Tensor
    time_to_collision: Tensor
    distance_to_road_edge: Optional[Tensor]
    offroad_per_step: Optional[Tensor]
    num_placement: Tensor                # [B][T2] int64
    num_removement: Tensor
    distance_placement: Tensor           # [B][N][T2]
    distance_removement: Tensor
    n_rows: Tensor
    bundle: Tensor
    n_scenario: int = 0
    n_rollout: int = 0
    rows_host: tuple = ()                # the row count per scenario as the host knows it (no copy to read it)
    bundle_rows_host: tuple = ()         # ... and per bundle (`n_rows` on the host)

    def rollout(self, b: int) -> MetricFeatures:
        """the MetricFeatures of bundle ``b`` (its real rows), as `compute_metric_features` returns them for that rollout"""
        n = self.bundle_rows_host[b]
        cut = lambda t: None if t is None else t[b, :n]
        per_object = ('object_id', 'valid', 'linear_speed', 'linear_acceleration', 'angular_speed', 'angular_acceleration',
                      'distance_to_nearest_object', 'collision_per_step', 'time_to_collision', 'distance_to_road_edge',
                      'offroad_per_step', 'distance_placement', 'distance_removement')
        return MetricFeatures(num_placement=self.num_placement[b][None], num_removement=self.num_removement[b][None],
                              **{k: cut(getattr(self, k)) for k in per_object})


def align_rollouts(rollouts: Sequence[Dict[str, Tensor]], return_counts: bool = False):
    """the per-copy dicts of `InfGenDecoder.inference_rollouts` with insertion hold different row counts (every copy inserts its
    own agents), which `format_rollouts` cannot stack.  -> dicts of equal layout: every graph gets the largest row count any copy
    has for it; a copy's missing rows are appended to that graph as padding (never valid, state 0 = `invalid`, agent_id -1).
    Dicts that already agree are returned as they are (no copy).  Single-graph dicts (no `agent_ptr`) are padded at their end;
    their row counts are shapes, so they cost no host read.
    ``return_counts``: -> (dicts, rows per graph, rows per graph and copy [B][n]) as host ints - the `agent_count` and
    `rollout_rows` `compute_metric_features_batch` lays its arrays out by, so that a copy's padding rows are not scored as
    objects; a multi-graph dict then always costs one host read of its `agent_ptr`s (`to_host`)."""
    keys = ('pred_valid', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_z', 'eval_shape', 'pred_type', 'next_state_idx',
            'agent_id')

    def padded(r, total, dest):
        """the row arrays of copy ``r`` laid out over ``total`` rows, its rows at ``dest``"""
        o = dict(r)
        for k in keys:
            v = r[k]
            pad = torch.full((total,) + tuple(v.shape[1:]), -1 if k == 'agent_id' else 0, dtype=v.dtype, device=v.device)
            pad[dest] = v
            o[k] = pad
        return o

    first = rollouts[0]
    sizes = [int(r['pred_traj'].shape[0]) for r in rollouts]
    same = len(set(sizes)) == 1
    if 'agent_ptr' not in first:
        top = max(sizes)
        out = [r if n == top else padded(r, top, slice(0, n)) for r, n in zip(rollouts, sizes)]
        return (out, [top], [sizes]) if return_counts else out
    if same and not return_counts:
        return list(rollouts)
    dev = first['pred_traj'].device
    ptr = to_host(torch.stack([r['agent_ptr'].long() for r in rollouts]))              # [n][B + 1], the one host read
    cnt = ptr[:, 1:] - ptr[:, :-1]
    top = cnt.max(0).values
    counts, per_copy = [int(c) for c in top], cnt.T.tolist()
    if bool((cnt == top[None]).all()):
        return (list(rollouts), counts, per_copy) if return_counts else list(rollouts)
    new_ptr = torch.cat([torch.zeros(1, dtype=torch.long), top.cumsum(0)])
    total, B = int(new_ptr[-1]), top.numel()
    out = []
    for j, r in enumerate(rollouts):
        g = r['agent_batch'].long()
        shift = (new_ptr[:-1] - ptr[j, :-1]).to(dev)                                   # how far graph g's rows move down
        o = padded(r, total, torch.arange(g.numel(), device=dev) + shift[g])
        o['agent_ptr'] = new_ptr.to(dev)
        o['agent_batch'] = torch.repeat_interleave(torch.arange(B, device=dev), top.to(dev), output_size=total)
        o['ego_index'] = torch.as_tensor(r['ego_index']).reshape(-1).long().to(dev) + shift
        out.append(o)
    return (out, counts, per_copy) if return_counts else out


def bundle_road_edges(road_edge_polylines, n_rollout: int, device):
    """road edges of a batch: one entry per scenario - a list of polylines or the (padded, cyclic) pair of
    `map_features.tensorize_polylines` - -> (polylines [P][L][4], cyclic [P], poly_off [B + 1]) for infgen_distance_to_road_edge,
    a scenario's polylines repeated for each of its rollouts (the entry takes one contiguous range per scene).  Host-side, once
    per batch."""
    pairs = [p if isinstance(p, tuple) and torch.is_tensor(p[0]) else map_features.tensorize_polylines(p)
             for p in road_edge_polylines]
    L = max(int(p.shape[1]) for p, _ in pairs)
    polys, cycs, off = [], [], [0]
    for p, c in pairs:
        p = torch.nn.functional.pad(p.float(), (0, 0, 0, L - p.shape[1]))
        for _ in range(n_rollout):
            polys.append(p)
            cycs.append(c.to(torch.uint8))
            off.append(off[-1] + p.shape[0])
    return (torch.cat(polys).to(device).contiguous(), torch.cat(cycs).to(device).contiguous(),
            torch.tensor(off, dtype=torch.int32).to(device), L)


@torch.no_grad()
def compute_metric_features_batch(rollouts: Dict, road_edge_polylines=None) -> MetricFeaturesBatch:
    """`compute_metric_features` of every rollout of every scenario of a rollouts dict (`format_rollouts`), without a
    per-scenario `ObjectTrajectories`: the dict's rows are scattered into padded [B][N_max][T] arrays and every feature is ONE
    launch of its library entry for the whole batch, whatever the number of scenarios and rollouts.
    The padded layout needs the row count per scenario on the host: it is taken from `rollouts['agent_count']` (a sequence of
    ints, as `InfGen.validation_step` adds it) or from a host-resident `agent_batch`; only a device-resident `agent_batch`
    without `agent_count` costs a host read (`to_host`).  A supplied `agent_count` is checked against the number of scenarios and
    rows only (anything more would be a host read): that it lists the scenarios in `agent_batch`'s numbering is the caller's
    part.  `rollouts['rollout_rows']` ([n_scenario][n_rollout] host ints, optional, from `align_rollouts`): how many of a
    scenario's rows exist in each rollout - the rest of that rollout's rows are padding and are left out of `n_rows`.
    `road_edge_polylines`: one entry per scenario (`bundle_road_edges`).
    The ego of a scenario is looked up on the device; an `av_id` no row carries selects row 0 instead of raising."""
    from .. import _lib
    traj = rollouts['pred_traj']
    dev = traj.device
    if dev.type != 'cuda':
        raise RuntimeError('compute_metric_features_batch runs on the GPU only (no CPU fallback)')
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    n, R, T = traj.shape[:3]
    S = int(rollouts['scenario_id'].shape[0])
    batch = rollouts['agent_batch']
    if 'agent_count' in rollouts:
        rows_host = tuple(int(c) for c in rollouts['agent_count'])
    else:
        counts = torch.bincount(batch.long(), minlength=S)
        rows_host = tuple(int(c) for c in (counts if counts.device.type == 'cpu' else to_host(counts)))
    assert len(rows_host) == S and sum(rows_host) == n, 'agent_count does not match agent_batch / scenario_id'
    N, B = max(max(rows_host), 1), S * R
    batch = batch.to(dev).long()
    order = torch.argsort(batch, stable=True)
    sb = batch[order]
    ptr = torch.tensor([0] + list(rows_host), device=dev).cumsum(0)
    local = torch.arange(n, device=dev) - ptr[sb]
    dest = ((sb[:, None] * R + torch.arange(R, device=dev)[None]) * N + local[:, None]).reshape(-1)      # [n * R] rows of [B * N]

    def pad(src: Tensor, dtype, fill=0) -> Tensor:
        """[n][R][...] rows of the dict -> [B][N][...]"""
        tail = tuple(src.shape[2:])
        out = torch.full((B * N,) + tail, fill, dtype=dtype, device=dev)
        out[dest] = src.to(dev)[order].reshape((n * R,) + tail).to(dtype)
        return out.reshape((B, N) + tail)

    f32 = torch.float32
    x, y = pad(traj[..., 0], f32), pad(traj[..., 1], f32)
    z, hd = pad(rollouts['pred_z'], f32), pad(rollouts['pred_head'], f32)
    shape = pad(rollouts['pred_shape'], f32)
    ln, wd, ht = (shape[..., k, None].expand(B, N, T).contiguous() for k in range(3))
    vd = pad(rollouts['pred_valid'], torch.uint8)
    object_id = pad(rollouts['agent_id'], rollouts['agent_id'].dtype, -1)
    tok = rollouts['token_pos']
    T2 = tok.shape[2]
    tx, ty = pad(tok[..., 0], f32), pad(tok[..., 1], f32)
    state = pad(rollouts['pred_state'], torch.int32, AGENT_STATE.index('invalid')) if 'pred_state' in rollouts else \
        torch.zeros(B, N, T2, dtype=torch.int32, device=dev)
    if rollouts.get('rollout_rows') is not None:
        bundle_rows = tuple(int(c) for per in rollouts['rollout_rows'] for c in per)
        assert len(bundle_rows) == B and all(0 <= c <= rows_host[b // R] for b, c in enumerate(bundle_rows)), \
            'rollout_rows: one count per scenario and rollout, none above agent_count'
    else:
        bundle_rows = tuple(c for c in rows_host for _ in range(R))
    n_rows = torch.tensor(bundle_rows, dtype=torch.int32, device=dev)
    bundle = torch.arange(S, device=dev).repeat_interleave(R)
    P = _lib.ptr
    cut = CURRENT_TIME_INDEX + 1
    # kinematics: one launch over the B * N rows (and one more for the planar speed the time-to-collision reads, like the
    # per-rollout wrapper's)
    kin = [torch.empty_like(x) for _ in range(4)]
    _lib.check(lib.infgen_kinematic_features(P(x), P(y), P(z), P(hd), B * N, T, STEP_DURATION_SECONDS, *(P(o) for o in kin),
                                             stream), 'infgen_kinematic_features')
    speed2 = torch.empty_like(x)
    flat = torch.zeros_like(x)
    _lib.check(lib.infgen_kinematic_features(P(x), P(y), P(flat), P(hd), B * N, T, STEP_DURATION_SECONDS, P(speed2), None, None,
                                             None, stream), 'infgen_kinematic_features')
    dist = torch.empty(B, N, T, device=dev)
    work = torch.empty(B * N * T * 9, device=dev)
    _lib.check(lib.infgen_distance_to_nearest_object(P(x), P(y), P(ln), P(wd), P(hd), P(vd), B, N, T, N,
                                                     interact_features.CORNER_ROUNDING_FACTOR, P(work), P(dist), stream),
               'infgen_distance_to_nearest_object')
    every = torch.arange(N, dtype=torch.int32, device=dev)
    ttc = torch.empty(B, N, T, device=dev)
    _lib.check(lib.infgen_time_to_collision(P(x), P(y), P(ln), P(wd), P(hd), P(speed2), P(vd), P(every), B, N, T, N, P(ttc),
                                            stream), 'infgen_time_to_collision')
    road = offroad = None
    if road_edge_polylines is not None:
        assert len(road_edge_polylines) == S, 'road_edge_polylines: one entry per scenario'
        poly, cyc, off, L = bundle_road_edges(road_edge_polylines, R, dev)
        road_all = torch.empty(B, N, T, device=dev)
        every_b = every.repeat(B).contiguous()
        _lib.check(lib.infgen_distance_to_road_edge(P(x), P(y), P(z), P(ln), P(wd), P(ht), P(hd), P(vd), P(every_b), B, N, T, N,
                                                    P(poly), P(cyc), P(off), L, map_features._Z_STRETCH_FACTOR, P(road_all),
                                                    stream), 'infgen_distance_to_road_edge')
        road = road_all[:, :, cut:]
        offroad = road > map_features.OFFROAD_DISTANCE_THRESHOLD
    n10 = T - cut
    av_id = rollouts.get('av_id', -1)
    if not torch.is_tensor(av_id) and int(av_id) == -1:
        num_in = torch.zeros(B, n10 // SHIFT, device=dev)
        num_out = num_in.clone()
        d_in = torch.zeros(B, N, n10 // SHIFT, device=dev)
        d_out = d_in.clone()
    else:
        av = torch.as_tensor(av_id, device=dev).reshape(-1).long().expand(S).repeat_interleave(R)
        av_index = (object_id == av[:, None]).int().argmax(1).to(torch.int32).contiguous()
        nb = torch.empty(B, T2, dtype=torch.int32, device=dev)
        ne = torch.empty_like(nb)
        db = torch.empty(B, N, T2, device=dev)
        de = torch.empty_like(db)
        _lib.check(lib.infgen_placement_features(P(tx), P(ty), None, P(state), P(av_index), B, N, T2, AGENT_STATE.index('enter'),
                                                 AGENT_STATE.index('exit'), P(nb), P(ne), P(db), P(de), stream),
                   'infgen_placement_features')
        c2 = CURRENT_TIME_INDEX // SHIFT
        num_in, num_out = nb.long()[:, c2:], ne.long()[:, c2:]
        d_in, d_out = db[:, :, c2:], de[:, :, c2:]
    # (compared before the cut, so the mask is a view of the same row stride as the features)
    collision = (dist < COLLISION_DISTANCE_THRESHOLD)[:, :, cut:]
    dist = dist[:, :, cut:]
    return MetricFeaturesBatch(
        object_id=object_id, valid=vd.bool()[:, :, cut:], linear_speed=kin[0][:, :, cut:], linear_acceleration=kin[1][:, :, cut:],
        angular_speed=kin[2][:, :, cut:], angular_acceleration=kin[3][:, :, cut:], distance_to_nearest_object=dist,
        collision_per_step=collision, time_to_collision=ttc[:, :, cut:], distance_to_road_edge=road,
        offroad_per_step=offroad, num_placement=num_in, num_removement=num_out, distance_placement=d_in,
        distance_removement=d_out, n_rows=n_rows, bundle=bundle, n_scenario=S, n_rollout=R, rows_host=rows_host,
        bundle_rows_host=bundle_rows)


def __getattr__(name):
    # the reference keeps LongMetric in this module (infgen/metrics/compute_metrics.py:1105); here it lives in long_metric.py,
    # which imports from this file - resolved on first use
    if name in ('LongMetric', 'compute_log_distributions', 'get_log_distributions'):
        from . import long_metric
        return getattr(long_metric, name)
    raise AttributeError(name)
