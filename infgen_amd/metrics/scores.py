"""Scoring stage of the reference's LongMetric on the device: mirror of compute_scenario_metrics_for_bundle
(infgen/metrics/compute_metrics.py:880-1103) from MetricFeatures to the per-feature likelihoods and the meta-metric.
The windowed histogram log-likelihoods (the reference's unfold + vmap(torch.histogram) + Categorical.log_prob + masked mean)
are one launch of `infgen_window_log_likelihood` per feature; what remains is arithmetic on (objects x windows) arrays.

`config`: the reference's SimAgentMetricsConfig (protobuf) or any object / dict with the same fields per feature
(`histogram.{min_val, max_val, num_bins}` or `bernoulli`, `metametric_weight`).  `log_distributions`: per feature a
torch.distributions.Categorical (as the reference's LogDistributions holds) or a tensor of log-probabilities."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from .. import _lib
from . import compute_metrics as _cm
from .compute_metrics import SHIFT, MetricFeatures, MetricFeaturesBatch

N_SIMULATION_STEPS = 80          # waymo_open_dataset submission_specs
KINEMATIC = ('linear_speed', 'linear_acceleration', 'angular_speed', 'angular_acceleration')
FIELDS = KINEMATIC + ('distance_to_nearest_object', 'collision_indication', 'time_to_collision', 'num_placement',
                      'num_removement', 'distance_placement', 'distance_removement')


def _field(obj, name):
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


def _hist(config, field) -> Tuple[float, float, int, float]:
    fc = _field(config, field)
    if field == 'collision_indication':
        return -0.5, 0.5, 2, float(_field(fc, 'metametric_weight'))
    h = _field(fc, 'histogram')
    return float(_field(h, 'min_val')), float(_field(h, 'max_val')), int(_field(h, 'num_bins')), float(_field(fc, 'metametric_weight'))


def _logp(log_distributions, field, dev) -> Tensor:
    d = _field(log_distributions, field)
    lp = d.logits if hasattr(d, 'logits') else torch.as_tensor(d)
    return lp.reshape(-1).to(dev, torch.float32).contiguous()


def window_log_likelihood(values: Tensor, valid, lo: float, hi: float, num_bins: int, logp: Tensor, size: int, step: int):
    """values / valid (n, T) on the GPU -> (sum of log-probabilities over the valid steps, number of valid steps) per
    (n, window)"""
    dev = values.device
    if dev.type != 'cuda':
        raise RuntimeError('window_log_likelihood runs on the GPU only (no CPU fallback)')
    v = values.to(torch.float32).contiguous()
    ok = valid.to(torch.uint8).contiguous() if valid is not None else None
    n, T = v.shape
    W = (T - size) // step + 1
    edges = torch.linspace(lo, hi, num_bins + 1).float().to(dev)          # the reference's edges, computed the same way
    s = torch.empty(n, W, dtype=torch.float32, device=dev)
    c = torch.empty(n, W, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().infgen_window_log_likelihood(_lib.ptr(v), _lib.ptr(ok), n, T, size, step, _lib.ptr(edges),
                                                       _lib.ptr(logp), num_bins, _lib.ptr(s), _lib.ptr(c),
                                                       torch.cuda.current_stream(dev).cuda_stream),
               'infgen_window_log_likelihood')
    return s, c


def _masked_mean(t: Tensor, dim=None) -> Tensor:
    """reference _reduce_mean (:765-774): mean over the entries in (0, 1]"""
    ok = (t > 0) & (t <= 1)
    z = torch.where(ok, t, torch.zeros_like(t))
    return z.sum() / ok.sum().clamp(min=1) if dim is None else z.sum(0) / ok.sum(0).clamp(min=1)


@torch.no_grad()
def compute_scenario_metrics(config, log_distributions, features: MetricFeatures, size: int = N_SIMULATION_STEPS,
                             step: int = SHIFT) -> Tuple[Dict[str, float], Dict[str, Tensor]]:
    """reference compute_metrics.py:880-1103 for one rollout's MetricFeatures -> (the SimAgentMetrics fields as floats:
    `<feature>_likelihood`, `metametric`, `simulated_collision_rate`; the per-window tensors (1, n_window) of the second
    return value of the reference)."""
    f = features
    valid = f.valid
    dev = valid.device
    sv = torch.zeros_like(valid)
    sv[:, 1:-1] = valid[:, 2:] & valid[:, :-2]                           # compute_kinematic_validity
    av = torch.zeros_like(valid)
    av[:, 1:-1] = sv[:, 2:] & sv[:, :-2]

    def score(field, values, ok, sz, stp):
        lo, hi, nb, _ = _hist(config, field)
        s, c = window_log_likelihood(values, ok, lo, hi, nb, _logp(log_distributions, field, dev), sz, stp)
        return s, c

    def likelihood(field, values, ok, sz=size, stp=step):
        s, c = score(field, values, ok, sz, stp)
        if int(c.sum()) == 0:
            return torch.zeros_like(s)                                  # exp(-inf), :759-760
        return torch.exp(s / c)                                          # 0 / 0 = NaN for a window without a valid step

    per = {}
    for k, ok in zip(KINEMATIC, (sv, av, sv, av)):
        per[k] = likelihood(k, getattr(f, k), ok)
    d = f.distance_to_nearest_object
    lo, hi, _, _ = _hist(config, 'distance_to_nearest_object')
    per['distance_to_nearest_object'] = likelihood('distance_to_nearest_object', d, valid & (d >= lo) & (d <= hi))
    per['time_to_collision'] = likelihood('time_to_collision', f.time_to_collision, valid)
    tok_valid = valid[:, ::SHIFT]
    for k in ('distance_placement', 'distance_removement'):
        d = getattr(f, k)
        lo, hi, _, _ = _hist(config, k)
        per[k] = likelihood(k, d, tok_valid[:, :d.shape[1]] & (d > lo) & (d < hi), size // SHIFT, step // SHIFT)
    scal = {k: _masked_mean(v) for k, v in per.items()}
    long = {k: _masked_mean(v, 0)[None] for k, v in per.items()}
    # collision indication per (object, window): any valid colliding step; bernoulli = two bins around 0 and 1
    hit_cnt = score('collision_indication', f.collision_per_step.float(), valid & f.collision_per_step, size, step)[1]
    hit = (hit_cnt > 0).float()
    ll_hit, _ = score('collision_indication', hit.reshape(-1, 1), None, 1, 1)
    ll_hit = ll_hit.reshape(hit.shape)
    scal['collision_indication'] = _masked_mean(torch.exp(ll_hit.mean()))
    long['collision_indication'] = _masked_mean(torch.exp(ll_hit), 0)[None]
    for k in ('num_placement', 'num_removement'):
        s, c = score(k, getattr(f, k).float(), None, size // SHIFT, step // SHIFT)
        scal[k] = _masked_mean(torch.exp(s.sum() / c.sum()))
        long[k] = torch.exp(s / c)
    weights = {k: _hist(config, k)[3] for k in FIELDS}
    out = {k + '_likelihood': float(scal[k]) for k in FIELDS}
    out['metametric'] = sum(weights[k] * out[k + '_likelihood'] for k in FIELDS)
    out['simulated_collision_rate'] = float(hit.mean())
    meta_long = sum(weights[k] * long[k][0] for k in FIELDS)
    for k in FIELDS:
        meta_long = torch.where(long[k][0] == 0, torch.zeros_like(meta_long), meta_long)
    long_out = {k + '_likelihood': long[k] for k in FIELDS}
    long_out['metametric'] = meta_long[None]
    return out, long_out


# ------------------------------------------------------------------------------------------------------------------------
# all rollouts of all scenarios of a batch in one call: infgen_bundle_scores (csrc/bundle_scores.hip)
TABLE_STRIDE = 136           # BS_TABLE_STRIDE of csrc/kernels.h: num_bins, min_val, max_val, weight, edges[65], logp[64], 3 unused
N_SCALAR = len(FIELDS) + 2   # the likelihoods, metametric, simulated_collision_rate


def pack_score_table(config, log_distributions, device) -> Tensor:
    """the histograms of every field as the one table infgen_bundle_scores reads (include/infgen_hip.h): built once per
    LongMetric.  The edges are the float32 linspace `window_log_likelihood` hands to the per-feature kernel."""
    tab = torch.zeros(len(FIELDS), TABLE_STRIDE)
    for i, k in enumerate(FIELDS):
        lo, hi, nb, w = _hist(config, k)
        if not 1 <= nb <= 64:
            raise ValueError(f'{k}: num_bins must be in 1..64')
        tab[i, 0], tab[i, 1], tab[i, 2], tab[i, 3] = nb, lo, hi, w
        tab[i, 4:5 + nb] = torch.linspace(lo, hi, nb + 1).float()
        tab[i, 69:69 + nb] = _logp(log_distributions, k, torch.device('cpu'))
    return tab.to(device).contiguous()


@dataclass(frozen=True)
class BundleScores:
    """device results of `compute_scenario_metrics_batch`: views of ONE buffer (`flat`), so one copy brings all to the host"""
    scalars: Tensor              # [n_scenario][13]: FIELDS' likelihoods, metametric, simulated_collision_rate
    long: Tensor                 # [n_scenario][12][n_window]: FIELDS' per-window likelihoods (the counts': rollout 0's), metametric
    long_rollout: Tensor         # [n_scenario][n_rollout][2][n_window]: num_placement / num_removement per rollout
    counters: Tensor             # [3] int32: scenarios, scenarios with a placement score, with a removement score
    flat: Tensor

    def to_dicts(self) -> List[Tuple[Dict[str, float], Dict[str, Tensor]]]:
        """per scenario the `(scalars, per-window)` pair of `compute_scenario_metrics` - with the reference's bundle shapes: the
        per-window values are (1, n_window), those of num_placement / num_removement (n_rollout, n_window) - after ONE host
        copy for the whole batch"""
        host = _cm.to_host(self.flat)
        S, _, W = self.long.shape
        R = self.long_rollout.shape[1]
        a, b = S * N_SCALAR, S * N_SCALAR + S * (len(FIELDS) + 1) * W
        scal = host[:a].reshape(S, N_SCALAR)
        long = host[a:b].reshape(S, len(FIELDS) + 1, W)
        per = host[b:b + S * R * 2 * W].reshape(S, R, 2, W)
        out = []
        for s in range(S):
            sc = {k + '_likelihood': float(scal[s, i]) for i, k in enumerate(FIELDS)}
            sc['metametric'] = float(scal[s, len(FIELDS)])
            sc['simulated_collision_rate'] = float(scal[s, len(FIELDS) + 1])
            lg = {k + '_likelihood': long[s, i][None].clone() for i, k in enumerate(FIELDS)}
            lg['num_placement_likelihood'] = per[s, :, 0].clone()
            lg['num_removement_likelihood'] = per[s, :, 1].clone()
            lg['metametric'] = long[s, len(FIELDS)][None].clone()
            out.append((sc, lg))
        return out


def _rows(t: Tensor):
    """-> (tensor, row stride in elements) of a [B][N][n] or [B][n] array whose rows are dense and evenly spaced; a column slice
    of a contiguous array qualifies as it is, anything else is copied"""
    ld = t.stride(-2)
    if not (t.stride(-1) == 1 and ld >= t.shape[-1] and (t.dim() == 2 or t.stride(0) == t.shape[1] * ld)):
        t = t.contiguous()
        ld = t.shape[-1]
    return t, ld


def _row_group(tensors, dtypes):
    """arrays that share one row stride for the library (made dense if they come as views of differently shaped parents)
    -> (tensors to keep alive, addresses, row stride)"""
    ts = [t.view(torch.uint8) if t.dtype == torch.bool and d == torch.uint8 else t.to(d) for t, d in zip(tensors, dtypes)]
    got = [_rows(t) for t in ts]
    if len({ld for _, ld in got}) > 1:
        got = [(t.contiguous(), t.shape[-1]) for t in ts]
    return [t for t, _ in got], [t.data_ptr() for t, _ in got], got[0][1]


@torch.no_grad()
def compute_scenario_metrics_batch(config, log_distributions, features: MetricFeaturesBatch, size: int = N_SIMULATION_STEPS,
                                   step: int = SHIFT, table: Optional[Tensor] = None, as_dicts: bool = False):
    """`compute_scenario_metrics` with the reference's bundle semantics (compute_scenario_metrics_for_bundle, :891-1103: the
    features of all rollouts of a scenario concatenated along the objects) for every scenario of a `MetricFeaturesBatch`, in
    ONE library call whatever the number of scenarios and rollouts.  -> `BundleScores` (device tensors; nothing is read back),
    or with ``as_dicts`` the per-scenario `(scalars dict, per-window dict)` list after one host copy.  ``table``: the result of
    `pack_score_table` when the caller keeps it (LongMetric does)."""
    f = features
    dev = f.valid.device
    if dev.type != 'cuda':
        raise RuntimeError('compute_scenario_metrics_batch runs on the GPU only (no CPU fallback)')
    if table is None:
        table = pack_score_table(config, log_distributions, dev)
    S, R = f.n_scenario, f.n_rollout
    B, N, T = f.valid.shape
    keep10, p10, ld = _row_group([f.valid, f.collision_per_step, f.linear_speed, f.linear_acceleration, f.angular_speed,
                                  f.angular_acceleration, f.distance_to_nearest_object, f.time_to_collision],
                                 [torch.uint8] * 2 + [torch.float32] * 6)
    T2 = f.distance_placement.shape[-1]
    keep_d, p_d, ld2 = _row_group([f.distance_placement, f.distance_removement], [torch.float32] * 2)
    keep_n, p_n, ldn = _row_group([f.num_placement, f.num_removement], [torch.int64] * 2)
    W = (T - size) // step + 1
    n_scal, n_long, n_per = S * N_SCALAR, S * (len(FIELDS) + 1) * W, B * 2 * W
    flat = torch.empty(n_scal + n_long + n_per + 3, dtype=torch.float32, device=dev)
    base = flat.data_ptr()
    n_rows = f.n_rows.to(torch.int32).contiguous()
    _lib.check(_lib.load().infgen_bundle_scores(
        *p10, *p_d, *p_n, _lib.ptr(n_rows), _lib.ptr(table), S, R, N, T, ld, T2, ld2, ldn, size, step, SHIFT, base,
        base + 4 * n_scal, base + 4 * (n_scal + n_long), base + 4 * (n_scal + n_long + n_per), torch.cuda.current_stream(dev).cuda_stream), 'infgen_bundle_scores')
    res = BundleScores(scalars=flat[:n_scal].view(S, N_SCALAR), long=flat[n_scal:n_scal + n_long].view(S, len(FIELDS) + 1, W),
                       long_rollout=flat[n_scal + n_long:n_scal + n_long + n_per].view(S, R, 2, W),
                       counters=flat[n_scal + n_long + n_per:].view(torch.int32), flat=flat)
    return res.to_dicts() if as_dicts else res
