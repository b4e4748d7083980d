"""``torch.library`` registration of the hot-path operators (last row): namespace ``infgen_hip``.

Every op is a thin binding of an ``extern "C"`` entry of libinfgen_hip.so (include/infgen_hip.h) - tensors are borrowed, outputs
are allocated here, launches go to torch's current HIP stream, errors surface as ``RuntimeError`` (``InfgenHipError``).  The ops
take the PACKED parameter blocks the library reads (``infgen_amd.packing``; the ``infgen_amd.modules`` layers pack their own
``state_dict`` parameters lazily), so a checkpoint is packed once and the ops are pure functions of tensors:

    torch.ops.infgen_hip.fourier_embed(x (E, n), pack, normalize)                          -> (E, 128)
    torch.ops.infgen_hip.radius_firstk(pos_q (Nq, 2), pos_x (Nx, 2), ptr_q, ptr_x, r, K)    -> idx (Nq, K) int32 (-1 padded), cnt (Nq,)
    torch.ops.infgen_hip.attn_layer(x_dst (N, 128), pack, off, cnt, src, rhat?, x_src?)     -> (N, 128)
    torch.ops.infgen_hip.token_state_head(x (N, 128), tok_pack, st_pack, token_size, want_logits) -> token, state, logits
    torch.ops.infgen_hip.token_logprob(logits (N, n), token (N,))                           -> (N,) log_softmax(logits)[token]; 0 where token < 0
    torch.ops.infgen_hip.heads_sample(x (N, 128), tok_pack, st_pack, token_size, k, uniform (N,), want_logits, want_logprob,
                                      want_sample_logprob, temperature=1, top_p=1, temperature_row=None)
                                                                                            -> token, state, logits, token_logprob, sample_logprob
    torch.ops.infgen_hip.sample_topk(logits (N, n), k, uniform (N,), want_sample_logprob, temperature=1, top_p=1,
                                     temperature_row=None)                                  -> token (N,), sample_logprob
    torch.ops.infgen_hip.collision_mask(pos, head, state, n_agents, type, shape, c, end_pose, predict=1, margin=0,
                                        mask_bits?, mask_row?, mask_type?, first_new?)      -> sets (S A, token_size / 32) int32, allowed (S A,)
    torch.ops.infgen_hip.road_mask(pos, head, state, n_agents, type, shape, c, end_pose, paths, records, n_records, copies=1,
                                   sweep=1, margin=0, types=[1, 0, 1], mask_bits?, mask_row?, mask_type?, first_new?)
                                                                                            -> sets (S A, token_size / 32) int32, allowed (S A,)
    torch.ops.infgen_hip.insert_cell_mask(pos, head, state, n_agents, av_index, shape, c, grid_xy, keepout?, clearance?,
                                          edge_clearance?, records?, n_records?, lane_dist?, lane_types?, map_pos?, map_type?, n_map?,
                                          zones?, n_zones?, copies=1)                       -> sets (S, W) int32, allowed (S,), live (S,)
    torch.ops.infgen_hip.route_mask(pos, head, state, n_agents, type, shape, c, end_pose, records, total, copies=1, corridor=2,
                                    back=0.5, pace=0, finish=1, types=[1, 0, 1], mask_bits?, mask_row?, mask_type?, first_new?)
                                                                                            -> sets, allowed (S A,), progress (S A, 4)
    torch.ops.infgen_hip.signal_mask(pos, head, state, n_agents, type, shape, c, end_pose, records, phase, t, copies=1,
                                     setback=0.5, align=0.5, types=[1, 0, 1], mask_bits?, mask_row?, mask_type?, first_new?)
                                                                                            -> sets, allowed (S A,), info (S A, 4)
    torch.ops.infgen_hip.step_score(pos, head, state, n_agents, type, shape, c1, records?, n_records?, copies=1, sweep=1,
                                    road_margin=0, types=[1, 0, 1], dt=0.5)                 -> score (S, 8), flags (S, A) uint8
    torch.ops.infgen_hip.observe_rows(pos, head, state, n_agents, type, shape, c, dt, map_pos?, map_orient?, map_type?, n_map?,
                                      copies=1, rows=None, neighbors=8, radius=None (inf), map_tokens=0, map_radius=None (inf))
                                                                                            -> self_feat (N, 8), nbr_feat (N, K, 10), nbr_index (N, K),
                                                                                               nbr_count (N,), map_feat (N, Km, 6), map_index (N, Km), map_count (N,)
    torch.ops.infgen_hip.idm_command(pos, head, state, n_agents, type, shape, ctl_row, c, records, total, cmd_pose, copies=1,
                                     v_des?, dt=0.5, v0=[15, 1.5, 6], headway=1.5, s_min=2, a_max=1.5, b_comf=2, b_max=6,
                                     lateral=0.5, keep=0.5, types=[1, 0, 1], stop_at_end=True)
                                                                                            -> state (S A, 8), lead (S A,); writes cmd_pose
    torch.ops.infgen_hip.map_token_head(x (N, 128), rows (n,), pack)                        -> logits (n, 1024), top-10 (n, 10) int64
    torch.ops.infgen_hip.mlp_layer(x (N, K), pack, n_out)                                   -> (N, n_out)
    torch.ops.infgen_hip.mlp_embedding(x (N, K), pack)                                      -> (N, 128)
    torch.ops.infgen_hip.bundle_scores(valid, collision, 4 kinematic, distance, ttc, 2 placement distances, 2 counts,
                                       n_rows, table, n_scenario, size, step, shift)        -> scalars, long, long_rollout, counters

    torch.ops.infgen_hip.integrate_tokenise(token, state, type, pos, head, n_agents, ego, vocab, grid) -> pos', head', pred_traj, pred_head, grid, state'
    torch.ops.infgen_hip.decode_step(ctx_bytes, t, pos, head, state, token, grid, x, next_token, next_state) -> next_token, next_state
    torch.ops.infgen_hip.command_rows(ctx_bytes, t, teacher_token, teacher_state, cmd_token?, cmd_pose?, cmd_mask?, shape?) -> cost (S, A_cap)
    torch.ops.infgen_hip.branch_scenes(ctx_bytes, t, parent (S,) int)                       -> n_bad (1,) int32; slot s := slot parent[s]
    torch.ops.infgen_hip.snapshot_scenes(ctx_bytes, t, slots (n,) int, snap (n, stride) uint8, head (n, 4) int32) -> n_bad; entry e := slot slots[e]
    torch.ops.infgen_hip.restore_scenes(ctx_bytes, t, index (S,) int, snap, head)           -> n_bad (1,) int32; slot s := entry index[s]
    torch.ops.infgen_hip.select_modes(traj (B, N, T, F), k, dist_thresh, scores?, valid?, t_goal=-1) -> mode_traj, mode_score, mode_idx (B, k)

(``decode_step`` works on the persistent state block ``InfgenRollout`` of include/infgen_hip.h, which ``RolloutEngine.ctx_tensor()``
hands out as bytes; whole rollouts stay a C-ABI call, ``infgen_rollout_run``, driven by infgen_amd/engine.py).  ``register_fake`` gives every op a shape function, so they trace under
``torch.compile`` / ``make_fx`` as opaque calls.  Inference only: no autograd formula is registered.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import _lib, controllers, observe
from .engine import Ops, D

_OPS = {}


def _ops(dev: torch.device) -> Ops:
    if dev.type != 'cuda':
        raise _lib.InfgenHipError('infgen_hip ops need cuda tensors: the HIP path has no CPU fallback')
    key = (dev.type, dev.index)
    if key not in _OPS:
        _OPS[key] = Ops(dev)
    return _OPS[key]


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().float()


def _sampling(temperature: float, top_p: float, temperature_row: Optional[torch.Tensor], rows: int, dev: torch.device):
    """-> (InfgenSampling, the per-row tensor it points at: keep it alive until the launch is enqueued)"""
    row = None
    if temperature_row is not None:
        if temperature_row.shape != (rows,):
            raise ValueError(f'temperature_row must hold one entry per row ({rows})')
        row = temperature_row.to(dev, torch.float32).contiguous()
    return _lib.Sampling(float(temperature), float(top_p), _lib.ptr(row)), row


@torch.library.custom_op('infgen_hip::fourier_embed', mutates_args=())
def fourier_embed(x: torch.Tensor, pack: torch.Tensor, normalize: bool = False) -> torch.Tensor:
    """FourierEmbedding.forward (reference infgen/modules/layers.py:142-160) of (E, n) continuous inputs, n <= 4; ``normalize``
    appends the affine-free LayerNorm the attention layers share (``attn_prenorm_r`` without gamma / beta)"""
    ops = _ops(x.device)
    n = x.shape[1]
    raw = torch.zeros(x.shape[0], 4, device=x.device)
    raw[:, :n] = x
    out = torch.empty(x.shape[0], D, device=x.device)
    if x.shape[0]:
        ops.fourier(raw, n, _f32(pack), out, normalize=normalize)
    return out


@fourier_embed.register_fake
def _(x, pack, normalize=False):
    return x.new_empty(x.shape[0], D, dtype=torch.float32)


@torch.library.custom_op('infgen_hip::radius_firstk', mutates_args=())
def radius_firstk(pos_q: torch.Tensor, pos_x: torch.Tensor, ptr_q: torch.Tensor, ptr_x: torch.Tensor, r: float,
                  K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch_cluster.radius(x=pos_x, y=pos_q, r, batch_x, batch_y, max_num_neighbors=K) for batches given as CSR pointers
    (agent_decoder.py:710-711 and the other call sites): per query the first K points of its batch in ascending index with
    d^2 < r^2, as a (Nq, K) index table padded with -1 and the per-query counts"""
    dev = pos_q.device
    ops = _ops(dev)
    nq, nx = pos_q.shape[0], pos_x.shape[0]
    idx = torch.full((nq, K), -1, device=dev, dtype=torch.int32)
    cnt = torch.zeros(nq, device=dev, dtype=torch.int32)
    if nq == 0 or nx == 0:
        return idx, cnt
    batch_q = torch.repeat_interleave(torch.arange(ptr_q.numel() - 1, device=dev), (ptr_q[1:] - ptr_q[:-1]).to(dev))
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    ar = torch.arange(nq, device=dev, dtype=torch.int32)
    c0, c1 = i32(ptr_x.to(dev)[batch_q]), i32(ptr_x.to(dev)[batch_q + 1])
    cap = nq * K
    off = torch.zeros(nq, device=dev, dtype=torch.int32)
    src = torch.zeros(cap, device=dev, dtype=torch.int32)
    raw = torch.empty(cap, 4, device=dev)
    total = torch.zeros(1, device=dev, dtype=torch.int32)
    zq, zx = torch.zeros(nq, device=dev), torch.zeros(nx, device=dev)
    a = _lib.RadiusEdges()
    P = _lib.ptr
    pq, px = _f32(pos_q), _f32(pos_x)
    a.n_q, a.q_node, a.q_pt, a.q_c0, a.q_c1 = nq, P(ar), P(ar), P(c0), P(c1)
    a.p_pos, a.p_head, a.c_pos, a.c_head = P(pq), P(zq), P(px), P(zx)
    a.radius, a.K = float(r), int(K)
    e = _lib.EdgeBuf()
    e.off, e.cnt, e.src, e.raw, e.total, e.cap = P(off), P(cnt), P(src), P(raw), P(total), cap
    _lib.check(ops.lib.infgen_radius_edges(C.byref(a), C.byref(e), ops.stream), 'infgen_radius_edges')
    pos = torch.arange(K, device=dev, dtype=torch.int32)[None, :]
    take = pos < cnt[:, None]
    gather = (off[:, None] + pos).clamp_(0, cap - 1).long()
    idx = torch.where(take, src[gather], idx)
    return idx, cnt


@radius_firstk.register_fake
def _(pos_q, pos_x, ptr_q, ptr_x, r, K):
    return pos_q.new_empty(pos_q.shape[0], K, dtype=torch.int32), pos_q.new_empty(pos_q.shape[0], dtype=torch.int32)


@torch.library.custom_op('infgen_hip::attn_layer', mutates_args=())
def attn_layer(x_dst: torch.Tensor, pack: torch.Tensor, off: torch.Tensor, cnt: torch.Tensor, src: torch.Tensor,
               rhat: Optional[torch.Tensor] = None, x_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """AttentionLayer.forward (reference infgen/modules/layers.py:61-113) on edges in CSR form by destination (``off`` / ``cnt``
    per destination row, ``src`` per edge indexes the source rows: of ``x_src`` for a bipartite layer, else of ``x_dst``);
    ``rhat`` (E, 128): normalised relative-position embedding of every edge (``fourier_embed(..., normalize=True)``)"""
    ops = _ops(x_dst.device)
    x = _f32(x_dst).clone()
    if x.shape[0]:
        ops.attention_layer(x, _f32(pack), off.int().contiguous(), cnt.int().contiguous(), src.int().contiguous(),
                            None if rhat is None else _f32(rhat), x_src=None if x_src is None else _f32(x_src))
    return x


@attn_layer.register_fake
def _(x_dst, pack, off, cnt, src, rhat=None, x_src=None):
    return torch.empty_like(x_dst, dtype=torch.float32)


@torch.library.custom_op('infgen_hip::token_state_head', mutates_args=())
def token_state_head(x: torch.Tensor, tok_pack: torch.Tensor, st_pack: torch.Tensor, token_size: int,
                     want_logits: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """token_predict_head / state_predict_head with the greedy arg-max (agent_decoder.py:2161-2167): next token (N,), next state
    (N,) and, on request, the (N, token_size) logits (else an empty tensor)"""
    ops = _ops(x.device)
    n = x.shape[0]
    tok = torch.zeros(n, device=x.device, dtype=torch.int32)
    st = torch.zeros(n, device=x.device, dtype=torch.int32)
    lg = torch.empty(n if want_logits else 0, token_size, device=x.device)
    if n:
        _lib.check(ops.lib.infgen_heads(_lib.ptr(_f32(x)), n, _lib.ptr(_f32(tok_pack)), _lib.ptr(_f32(st_pack)), int(token_size),
                                        _lib.ptr(lg) if want_logits else None, _lib.ptr(tok), _lib.ptr(st), ops.stream),
                   'infgen_heads')
    return tok, st, lg


@token_state_head.register_fake
def _(x, tok_pack, st_pack, token_size, want_logits=False):
    n = x.shape[0]
    return (x.new_empty(n, dtype=torch.int32), x.new_empty(n, dtype=torch.int32),
            x.new_empty(n if want_logits else 0, token_size, dtype=torch.float32))


@torch.library.custom_op('infgen_hip::token_logprob', mutates_args=())
def token_logprob(logits: torch.Tensor, token: torch.Tensor) -> torch.Tensor:
    """full-softmax log-probability of one token per row: ``logits[row, token[row]] - logsumexp(logits[row])`` in fp32
    (max-subtracted, fixed summation order: bitwise reproducible); rows whose token is negative give 0, a token of n or more gives
    NaN (checked by the kernel: no host synchronisation, so the op can be captured in a graph)"""
    if logits.dim() != 2 or token.shape != logits.shape[:1]:
        raise ValueError('token_logprob takes logits (N, n) and token (N,)')
    ops = _ops(logits.device)
    n = logits.shape[0]
    out = torch.zeros(n, device=logits.device)
    if n:
        lg, tok = _f32(logits), token.to(logits.device, torch.int32).contiguous()
        _lib.check(ops.lib.infgen_token_logprob(_lib.ptr(lg), n, int(lg.shape[1]), _lib.ptr(tok), _lib.ptr(out), ops.stream),
                   'infgen_token_logprob')
    return out


@token_logprob.register_fake
def _(logits, token):
    return logits.new_empty(logits.shape[0], dtype=torch.float32)


def _token_mask(mask_bits, mask_row, mask_type, agent_type, n: int, token_size: int, dev):
    """the ops' trailing mask arguments -> (the C entries' five mask arguments, tensors to keep alive): ``mask_bits`` (n_sets, token_size / 32)
    packed 32-bit words (infgen_amd.constraints.TokenMasks.bits), ``mask_row`` (N,) int set per row (-1: the type's), ``mask_type``
    three ints (-1: unconstrained), ``type`` (N,) int row types.  Shapes are checked here; set indices are the library's to read
    (one beyond the table means unconstrained)"""
    if mask_bits is None:
        if mask_row is not None or mask_type is not None:
            raise ValueError('mask_row / mask_type need mask_bits')
        return (None, 0, None, None, None), ()
    if token_size % 32 or mask_bits.dim() != 2 or mask_bits.shape[1] != token_size // 32 or mask_bits.element_size() != 4 \
            or mask_bits.is_floating_point():
        raise ValueError(f'mask_bits must be (n_sets, {token_size} / 32) 32-bit words')
    mt = [-1, -1, -1] if mask_type is None else [int(v) for v in mask_type]
    if len(mt) != 3:
        raise ValueError('mask_type takes three set indices (vehicle, pedestrian, cyclist; -1: unconstrained)')
    if any(v >= 0 for v in mt) and agent_type is None:
        raise ValueError('a per-type token mask needs the rows\' types')
    for name, t in (('mask_row', mask_row), ('type', agent_type)):
        if t is not None and tuple(t.shape) != (n,):
            raise ValueError(f'{name} must have one entry per row')
    bits = mask_bits.to(dev).contiguous()
    row = None if mask_row is None else mask_row.to(dev, torch.int32).contiguous()
    ty = None if agent_type is None else agent_type.to(dev, torch.int32).contiguous()
    return (_lib.ptr(bits), int(bits.shape[0]), _lib.ptr(row), (C.c_int * 3)(*mt), _lib.ptr(ty)), (bits, row, ty)


@torch.library.custom_op('infgen_hip::heads_sample', mutates_args=())
def heads_sample(x: torch.Tensor, tok_pack: torch.Tensor, st_pack: torch.Tensor, token_size: int, k: int, uniform: torch.Tensor,
                 want_logits: bool = False, want_logprob: bool = False, want_sample_logprob: bool = False,
                 temperature: float = 1.0, top_p: float = 1.0, temperature_row: Optional[torch.Tensor] = None,
                 mask_bits: Optional[torch.Tensor] = None, mask_row: Optional[torch.Tensor] = None,
                 mask_type: Optional[List[int]] = None, type: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """token_predict_head / state_predict_head with the motion token drawn by top-k sampling (agent_decoder.py:2162-2163, 2194-2195;
    ``infgen_heads_sample``): the ``k`` (1..16) best logits of a row in (value descending, column ascending) order, inverse CDF
    over their re-normalised probabilities with ``uniform[row]`` in [0, 1).  Returns next token (N,), next state (N,) and, each on
    request (else an empty tensor), the (N, token_size) logits, the full-softmax log-probability of the sampled token (N,) and its
    log-probability under the re-normalised top-k distribution (N,).  Where the library samples inside the split heads kernel
    (``infgen_heads_sample_fused``) no logit reaches memory unless asked for; elsewhere the op holds the logits itself.
    ``temperature`` / ``top_p`` / ``temperature_row`` (N,): temperature and nucleus truncation of the draw (``InfgenSampling`` of
    include/infgen_hip.h; a per-row temperature of 0 makes the row greedy); the full-softmax log-probability is not tempered.
    ``mask_bits`` / ``mask_row`` / ``mask_type`` / ``type``: per-row allowed-token sets (the token mask of include/infgen_hip.h; ``_token_mask``): a
    banned token is never emitted, the logits and the full-softmax log-probability stay the model's own"""
    if x.dim() != 2 or x.shape[1] != D or uniform.shape != x.shape[:1]:
        raise ValueError('heads_sample takes x (N, 128) and uniform (N,)')
    sp, _keep = _sampling(temperature, top_p, temperature_row, x.shape[0], x.device)
    tm, _keep_mask = _token_mask(mask_bits, mask_row, mask_type, type, x.shape[0], int(token_size), x.device)
    ops = _ops(x.device)
    n = x.shape[0]
    tok = torch.zeros(n, device=x.device, dtype=torch.int32)
    st = torch.zeros(n, device=x.device, dtype=torch.int32)
    o = _lib.Options()
    _lib.check(ops.lib.infgen_get_effective_options(C.byref(o)), 'infgen_get_effective_options')
    keep = want_logits or not ops.lib.infgen_heads_sample_fused(int(o.attn_mode), n, int(k))
    lg = torch.empty(n if keep else 0, token_size, device=x.device)
    lp = torch.zeros(n if want_logprob else 0, device=x.device)
    slp = torch.zeros(n if want_sample_logprob else 0, device=x.device)
    if n:
        u = uniform.to(x.device, torch.float32).contiguous()
        _lib.check(ops.lib.infgen_heads_sample_mask(_lib.ptr(_f32(x)), n, _lib.ptr(_f32(tok_pack)), _lib.ptr(_f32(st_pack)),
                                                    int(token_size), int(k), _lib.ptr(u), C.byref(sp),
                                                    *tm, _lib.ptr(lg) if keep else None,
                                                    _lib.ptr(tok), _lib.ptr(st), _lib.ptr(lp) if want_logprob else None,
                                                    _lib.ptr(slp) if want_sample_logprob else None, ops.stream),
                   'infgen_heads_sample_mask')
    return tok, st, (lg if want_logits else lg.new_empty(0, token_size)), lp, slp


@heads_sample.register_fake
def _(x, tok_pack, st_pack, token_size, k, uniform, want_logits=False, want_logprob=False, want_sample_logprob=False,
      temperature=1.0, top_p=1.0, temperature_row=None, mask_bits=None, mask_row=None, mask_type=None, type=None):
    n = x.shape[0]
    return (x.new_empty(n, dtype=torch.int32), x.new_empty(n, dtype=torch.int32),
            x.new_empty(n if want_logits else 0, token_size, dtype=torch.float32),
            x.new_empty(n if want_logprob else 0, dtype=torch.float32),
            x.new_empty(n if want_sample_logprob else 0, dtype=torch.float32))


@torch.library.custom_op('infgen_hip::sample_topk', mutates_args=())
def sample_topk(logits: torch.Tensor, k: int, uniform: torch.Tensor, want_sample_logprob: bool = False,
                temperature: float = 1.0, top_p: float = 1.0, temperature_row: Optional[torch.Tensor] = None,
                mask_bits: Optional[torch.Tensor] = None, mask_row: Optional[torch.Tensor] = None,
                mask_type: Optional[List[int]] = None, type: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """top-k sampling over stored logits (N, n) (``infgen_sample_topk_ex``; agent_decoder.py:2162-2163, 2194-2195): the ``k`` (1..16)
    best logits of a row, inverse CDF with ``uniform[row]``; ``temperature`` / ``top_p`` / ``temperature_row`` as in ``heads_sample``.
    Returns the token (N,) and, on request (else empty), its log-probability under the sampler's own distribution (N,).
    ``mask_bits`` / ``mask_row`` / ``mask_type`` / ``type`` as in ``heads_sample`` (``infgen_sample_topk_mask``; n a multiple of 32)"""
    if logits.dim() != 2 or uniform.shape != logits.shape[:1]:
        raise ValueError('sample_topk takes logits (N, n) and uniform (N,)')
    ops = _ops(logits.device)
    n = logits.shape[0]
    sp, _keep = _sampling(temperature, top_p, temperature_row, n, logits.device)
    tm, _keep_mask = _token_mask(mask_bits, mask_row, mask_type, type, n, int(logits.shape[1]), logits.device)
    tok = torch.zeros(n, device=logits.device, dtype=torch.int32)
    slp = torch.zeros(n if want_sample_logprob else 0, device=logits.device)
    if n:
        lg, u = _f32(logits), uniform.to(logits.device, torch.float32).contiguous()
        _lib.check(ops.lib.infgen_sample_topk_mask(_lib.ptr(lg), n, int(lg.shape[1]), int(k), _lib.ptr(u), C.byref(sp),
                                                   *tm, _lib.ptr(tok),
                                                   _lib.ptr(slp) if want_sample_logprob else None, None, ops.stream),
                   'infgen_sample_topk_mask')
    return tok, slp


@sample_topk.register_fake
def _(logits, k, uniform, want_sample_logprob=False, temperature=1.0, top_p=1.0, temperature_row=None, mask_bits=None, mask_row=None,
      mask_type=None, type=None):
    n = logits.shape[0]
    return logits.new_empty(n, dtype=torch.int32), logits.new_empty(n if want_sample_logprob else 0, dtype=torch.float32)


def collision_end_poses(vocab: torch.Tensor) -> torch.Tensor:
    """the end-pose table of ``collision_mask`` for a vocabulary (3, token_size, 6, 4, 2): 12 token_size + 4 floats
    (``infgen_collision_end_poses``; computed once per vocabulary)"""
    if vocab.dim() != 5 or tuple(vocab.shape[0:1] + vocab.shape[2:]) != (3, 6, 4, 2):
        raise ValueError('vocab must be (3, token_size, 6, 4, 2)')
    ops, n = _ops(vocab.device), int(vocab.shape[1])
    tab = torch.zeros(12 * n + 4, device=vocab.device)
    _lib.check(ops.lib.infgen_collision_end_poses(_lib.ptr(_f32(vocab)), n, _lib.ptr(tab), ops.stream), 'infgen_collision_end_poses')
    return tab


@torch.library.custom_op('infgen_hip::collision_mask', mutates_args=())
def collision_mask(pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, n_agents: torch.Tensor, type: torch.Tensor,
                   shape: torch.Tensor, c: int, end_pose: torch.Tensor, predict: int = 1, margin: float = 0.0,
                   mask_bits: Optional[torch.Tensor] = None, mask_row: Optional[torch.Tensor] = None,
                   mask_type: Optional[List[int]] = None, first_new: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """the allowed-token sets of one decode step from the agents' boxes (collision-aware decoding; "collision masks" of
    include/infgen_hip.h, ``infgen_collision_mask``): ``pos`` (S, T, A, 2), ``head`` / ``state`` (S, T, A), ``n_agents`` (S,),
    ``type`` (S, A), ``shape`` (S, A, 3) = length, width, height, column ``c``, ``end_pose`` from ``collision_end_poses``.
    ``mask_bits`` / ``mask_row`` (S * A,) / ``mask_type``: the static base sets (none: every token); ``first_new`` (S,): rows at or
    beyond it are not in the scene yet.  Returns the sets (S * A, token_size / 32) int32 words and the number of allowed tokens
    per row before the empty-set fallback (S * A,)."""
    if pos.dim() != 4 or pos.shape[3] != 2 or head.shape != pos.shape[:3] or state.shape != pos.shape[:3]:
        raise ValueError('collision_mask takes pos (S, T, A, 2), head (S, T, A), state (S, T, A)')
    S, T, A = (int(v) for v in pos.shape[:3])
    if tuple(type.shape) != (S, A) or tuple(shape.shape) != (S, A, 3) or tuple(n_agents.shape) != (S,):
        raise ValueError('collision_mask takes type (S, A), shape (S, A, 3), n_agents (S,)')
    if first_new is not None and tuple(first_new.shape) != (S,):
        raise ValueError('first_new must be (S,)')
    token_size = (int(end_pose.numel()) - 4) // 12
    if end_pose.dim() != 1 or token_size * 12 + 4 != end_pose.numel() or token_size % 32:
        raise ValueError('end_pose is the table of collision_end_poses (12 token_size + 4 floats, token_size a multiple of 32)')
    dev = pos.device
    ops = _ops(dev)
    i32 = lambda t: None if t is None else t.to(dev, torch.int32).contiguous()
    ty = i32(type)
    tm, _keep_mask = _token_mask(mask_bits, mask_row, mask_type, ty.reshape(-1), S * A, token_size, dev)
    bits = torch.zeros(S * A, token_size // 32, device=dev, dtype=torch.int32)
    count = torch.zeros(S * A, device=dev, dtype=torch.int32)
    st, na, fn = i32(state), i32(n_agents), i32(first_new)
    p, h, sh, ep = _f32(pos), _f32(head), _f32(shape), _f32(end_pose)
    _lib.check(ops.lib.infgen_collision_mask(_lib.ptr(p), _lib.ptr(h), _lib.ptr(st), _lib.ptr(na), _lib.ptr(fn), _lib.ptr(ty),
                                             _lib.ptr(sh), S, A, T, int(c), _lib.ptr(ep), token_size, int(predict), float(margin),
                                             *tm[:4], _lib.ptr(bits), _lib.ptr(count), ops.stream), 'infgen_collision_mask')
    return bits, count


@collision_mask.register_fake
def _(pos, head, state, n_agents, type, shape, c, end_pose, predict=1, margin=0.0, mask_bits=None, mask_row=None, mask_type=None,
      first_new=None):
    rows = pos.shape[0] * pos.shape[2]
    return (pos.new_empty(rows, (end_pose.shape[0] - 4) // 12 // 32, dtype=torch.int32), pos.new_empty(rows, dtype=torch.int32))


def road_paths(end_pose: torch.Tensor) -> torch.Tensor:
    """the path table of ``road_mask`` from the end-pose table of ``collision_end_poses``: (3, token_size, 4) = cos, sin of every
    token's end displacement, half its length, 0 (``infgen_road_paths``; computed once per vocabulary)"""
    n = (int(end_pose.numel()) - 4) // 12
    if end_pose.dim() != 1 or n * 12 + 4 != end_pose.numel() or n <= 0:
        raise ValueError('end_pose is the table of collision_end_poses (12 token_size + 4 floats)')
    ops = _ops(end_pose.device)
    ep, tab = _f32(end_pose), torch.zeros(3, n, 4, device=end_pose.device)
    _lib.check(ops.lib.infgen_road_paths(_lib.ptr(ep), n, _lib.ptr(tab), ops.stream), 'infgen_road_paths')
    return tab


def road_records_from_map(map_pos: torch.Tensor, map_orient: torch.Tensor, map_type: torch.Tensor, map_tok: torch.Tensor,
                          n_map: torch.Tensor, map_vocab: torch.Tensor, detail: int = 2,
                          capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """the road-segment records of S0 distinct scenes from their EDGE (type 12) map tokens ("road masks" of include/infgen_hip.h,
    ``infgen_road_records_from_map``): ``map_pos`` (S0, M, 2), ``map_orient`` / ``map_type`` / ``map_tok`` (S0, M), ``n_map`` (S0,),
    ``map_vocab`` (n_token, 11, 2) or (n_token, 22).  ``capacity``: records per scene (None: counted from ``map_type``, one
    synchronisation).  -> records (S0, capacity, 8), n_records (S0,) int32"""
    if map_pos.dim() != 3 or map_pos.shape[2] != 2 or any(tuple(t.shape) != tuple(map_pos.shape[:2]) for t in (map_orient, map_type, map_tok)):
        raise ValueError('road_records_from_map takes map_pos (S0, M, 2) and map_orient, map_type, map_tok (S0, M)')
    S0, M = (int(v) for v in map_pos.shape[:2])
    if tuple(n_map.shape) != (S0,) or map_vocab.numel() % 22 or map_vocab.numel() == 0:
        raise ValueError('road_records_from_map takes n_map (S0,) and map_vocab (n_token, 11, 2)')
    if detail not in (1, 2, 5, 10):
        raise ValueError('detail must be 1, 2, 5 or 10')
    dev = map_pos.device
    ops = _ops(dev)
    ty, tk = map_type.to(dev, torch.int64).contiguous(), map_tok.to(dev, torch.int64).contiguous()
    nm = n_map.to(dev, torch.int32).contiguous()
    if capacity is None:
        inmap = torch.arange(M, device=dev)[None] < nm[:, None]
        capacity = int(((ty == 12) & inmap).sum(dim=1).max().item()) * int(detail)
    cap = max(int(capacity), 1)
    rec, n = torch.zeros(S0, cap, 8, device=dev), torch.zeros(S0, device=dev, dtype=torch.int32)
    mp, mo, mv = _f32(map_pos), _f32(map_orient), _f32(map_vocab)
    _lib.check(ops.lib.infgen_road_records_from_map(_lib.ptr(mp), _lib.ptr(mo), _lib.ptr(ty), _lib.ptr(tk), _lib.ptr(nm), S0, M,
                                                    _lib.ptr(mv), int(mv.numel()) // 22, int(detail), _lib.ptr(rec), cap, _lib.ptr(n),
                                                    ops.stream), 'infgen_road_records_from_map')
    return rec, n


def road_records_from_segments(segments: torch.Tensor, n_segments: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """the records of explicit world-coordinate segments (S0, E, 4) = x0, y0, x1, y1, the first ``n_segments`` (S0,) of each scene
    (``infgen_road_records_from_segments``) -> records (S0, E, 8), n_records (S0,) int32"""
    if segments.dim() != 3 or segments.shape[2] != 4 or segments.shape[1] == 0 or tuple(n_segments.shape) != (segments.shape[0],):
        raise ValueError('road_records_from_segments takes segments (S0, E, 4) and n_segments (S0,)')
    dev = segments.device
    ops = _ops(dev)
    S0, E = (int(v) for v in segments.shape[:2])
    sg, ns = _f32(segments), n_segments.to(dev, torch.int32).contiguous()
    rec, n = torch.zeros(S0, E, 8, device=dev), torch.zeros(S0, device=dev, dtype=torch.int32)
    _lib.check(ops.lib.infgen_road_records_from_segments(_lib.ptr(sg), _lib.ptr(ns), S0, E, _lib.ptr(rec), E, _lib.ptr(n), ops.stream),
               'infgen_road_records_from_segments')
    return rec, n


@torch.library.custom_op('infgen_hip::road_mask', mutates_args=())
def road_mask(pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, n_agents: torch.Tensor, type: torch.Tensor,
              shape: torch.Tensor, c: int, end_pose: torch.Tensor, paths: torch.Tensor, records: torch.Tensor,
              n_records: torch.Tensor, copies: int = 1, sweep: int = 1, margin: float = 0.0, types: Optional[List[int]] = None,
              mask_bits: Optional[torch.Tensor] = None, mask_row: Optional[torch.Tensor] = None,
              mask_type: Optional[List[int]] = None, first_new: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """the allowed-token sets of one decode step from the road-edge records (road-aware decoding; "road masks" of
    include/infgen_hip.h, ``infgen_road_mask``): the scene arrays and ``end_pose`` as for ``collision_mask``, ``paths`` from
    ``road_paths``, ``records`` (S / copies, capacity, 8) and ``n_records`` (S / copies,) from ``road_records_from_map`` /
    ``_from_segments``, ``types`` the (vehicle, pedestrian, cyclist) switch (None: vehicles and cyclists).  ``mask_bits`` /
    ``mask_row`` / ``mask_type``: the base sets (none: every token).  Returns the sets (S * A, token_size / 32) int32 words and the
    number of allowed tokens per row before the empty-set fallback (S * A,)."""
    if pos.dim() != 4 or pos.shape[3] != 2 or head.shape != pos.shape[:3] or state.shape != pos.shape[:3]:
        raise ValueError('road_mask takes pos (S, T, A, 2), head (S, T, A), state (S, T, A)')
    S, T, A = (int(v) for v in pos.shape[:3])
    if tuple(type.shape) != (S, A) or tuple(shape.shape) != (S, A, 3) or tuple(n_agents.shape) != (S,):
        raise ValueError('road_mask takes type (S, A), shape (S, A, 3), n_agents (S,)')
    if first_new is not None and tuple(first_new.shape) != (S,):
        raise ValueError('first_new must be (S,)')
    token_size = (int(end_pose.numel()) - 4) // 12
    if end_pose.dim() != 1 or token_size * 12 + 4 != end_pose.numel() or token_size % 32:
        raise ValueError('end_pose is the table of collision_end_poses (12 token_size + 4 floats, token_size a multiple of 32)')
    if paths.numel() != 12 * token_size:
        raise ValueError('paths is the table of road_paths (3, token_size, 4)')
    if copies < 1 or S % copies:
        raise ValueError('copies must be at least 1 and divide S')
    if records.dim() != 3 or records.shape[2] != 8 or records.shape[0] != S // copies or tuple(n_records.shape) != (S // copies,):
        raise ValueError('road_mask takes records (S / copies, capacity, 8) and n_records (S / copies,)')
    types = [1, 0, 1] if types is None else [int(bool(v)) for v in types]
    if len(types) != 3:
        raise ValueError('types has three entries: vehicle, pedestrian, cyclist')
    dev = pos.device
    ops = _ops(dev)
    i32 = lambda t: None if t is None else t.to(dev, torch.int32).contiguous()
    ty = i32(type)
    tm, _keep_mask = _token_mask(mask_bits, mask_row, mask_type, ty.reshape(-1), S * A, token_size, dev)
    bits = torch.zeros(S * A, token_size // 32, device=dev, dtype=torch.int32)
    count = torch.zeros(S * A, device=dev, dtype=torch.int32)
    st, na, fn, nr = i32(state), i32(n_agents), i32(first_new), i32(n_records)
    p, h, sh, ep, pa, rc = _f32(pos), _f32(head), _f32(shape), _f32(end_pose), _f32(paths), _f32(records)
    _lib.check(ops.lib.infgen_road_mask(_lib.ptr(p), _lib.ptr(h), _lib.ptr(st), _lib.ptr(na), _lib.ptr(fn), _lib.ptr(ty), _lib.ptr(sh),
                                        S, A, T, int(c), _lib.ptr(ep), _lib.ptr(pa), token_size, _lib.ptr(rc), _lib.ptr(nr),
                                        int(records.shape[1]), int(copies), int(sweep), float(margin), (C.c_int * 3)(*types),
                                        *tm[:4], _lib.ptr(bits), _lib.ptr(count), ops.stream), 'infgen_road_mask')
    return bits, count


@road_mask.register_fake
def _(pos, head, state, n_agents, type, shape, c, end_pose, paths, records, n_records, copies=1, sweep=1, margin=0.0, types=None,
      mask_bits=None, mask_row=None, mask_type=None, first_new=None):
    rows = pos.shape[0] * pos.shape[2]
    return (pos.new_empty(rows, (end_pose.shape[0] - 4) // 12 // 32, dtype=torch.int32), pos.new_empty(rows, dtype=torch.int32))


@torch.library.custom_op('infgen_hip::insert_cell_mask', mutates_args=())
def insert_cell_mask(pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, n_agents: torch.Tensor, av_index: torch.Tensor,
                     shape: torch.Tensor, c: int, grid_xy: torch.Tensor, keepout: Optional[List[float]] = None,
                     clearance: Optional[float] = None, edge_clearance: Optional[float] = None,
                     records: Optional[torch.Tensor] = None, n_records: Optional[torch.Tensor] = None,
                     lane_dist: Optional[float] = None, lane_types: Optional[List[int]] = None,
                     map_pos: Optional[torch.Tensor] = None, map_type: Optional[torch.Tensor] = None,
                     n_map: Optional[torch.Tensor] = None, zones: Optional[torch.Tensor] = None,
                     n_zones: Optional[torch.Tensor] = None, copies: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the allowed cells of scenario insertion for column ``c`` (insertion rules; "INSERTION RULES" of include/infgen_hip.h,
    ``infgen_insert_cell_mask``): pos (S, T, A, 2), head / state (S, T, A), n_agents / av_index (S,), shape (S, A, 3), grid_xy
    (G, 2) in the ego frame.  A rule whose arguments are None is off: ``keepout`` (back, front, half_width); ``clearance``;
    ``edge_clearance`` with ``records`` (S / copies, capacity, 8) / ``n_records``; ``lane_dist`` with ``lane_types`` / ``map_pos``
    (S / copies, M, 2) / ``map_type`` (S / copies, M) / ``n_map``; ``zones`` (S / copies, Z, 4) / ``n_zones``.  Returns the sets
    (S, W) int32 words, W = ceil(G / 32) rounded up to a multiple of 4, the number of allowed cells (S,) and the number of rows in
    the scene at the column (S,)."""
    from . import insertion_rules as ir
    if pos.dim() != 4 or pos.shape[3] != 2 or head.shape != pos.shape[:3] or state.shape != pos.shape[:3]:
        raise ValueError('insert_cell_mask takes pos (S, T, A, 2), head (S, T, A), state (S, T, A)')
    S, T, A = (int(v) for v in pos.shape[:3])
    if tuple(shape.shape) != (S, A, 3) or tuple(n_agents.shape) != (S,) or tuple(av_index.shape) != (S,):
        raise ValueError('insert_cell_mask takes shape (S, A, 3), n_agents (S,), av_index (S,)')
    if grid_xy.dim() != 2 or grid_xy.shape[1] != 2:
        raise ValueError('grid_xy is (G, 2)')
    if copies < 1 or S % copies:
        raise ValueError('copies must be at least 1 and divide S')
    dev, G, S0 = pos.device, int(grid_xy.shape[0]), S // max(copies, 1)
    ops = _ops(dev)
    i32 = lambda t: None if t is None else t.to(dev, torch.int32).contiguous()
    rules = 0
    if keepout is not None:
        if len(keepout) != 3:
            raise ValueError('keepout has three entries: back, front, half_width')
        rules |= ir.KEEPOUT
    rules |= ir.CLEARANCE * (clearance is not None) | ir.EDGES * (edge_clearance is not None) | ir.LANES * (lane_dist is not None)
    rules |= ir.ZONES * (zones is not None)
    if edge_clearance is not None and (records is None or n_records is None or records.dim() != 3 or records.shape[2] != 8
                                       or records.shape[0] != S0 or tuple(n_records.shape) != (S0,)):
        raise ValueError('edge_clearance takes records (S / copies, capacity, 8) and n_records (S / copies,)')
    if lane_dist is not None and (map_pos is None or map_type is None or n_map is None or lane_types is None or map_pos.dim() != 3
                                  or map_pos.shape[0] != S0 or tuple(map_type.shape) != tuple(map_pos.shape[:2])
                                  or tuple(n_map.shape) != (S0,) or any(not 0 <= int(t) < 32 for t in lane_types)):
        raise ValueError('lane_dist takes lane_types in 0..31, map_pos (S / copies, M, 2), map_type (S / copies, M), n_map (S / copies,)')
    if zones is not None and (n_zones is None or zones.dim() != 3 or zones.shape[2] != 4 or zones.shape[0] != S0
                              or tuple(n_zones.shape) != (S0,)):
        raise ValueError('zones takes zones (S / copies, Z, 4) and n_zones (S / copies,)')
    W = ir.words_for(G)
    bits = torch.zeros(S, W, device=dev, dtype=torch.int32)
    count, live = torch.zeros(S, device=dev, dtype=torch.int32), torch.zeros(S, device=dev, dtype=torch.int32)
    p, h, sh, gx = _f32(pos), _f32(head), _f32(shape), _f32(grid_xy)
    st, na, av, nr, nm, nz = i32(state), i32(n_agents), i32(av_index), i32(n_records), i32(n_map), i32(n_zones)
    rc, mp, zn = (None if t is None else _f32(t) for t in (records, map_pos, zones))
    mt = None if map_type is None else map_type.to(dev, torch.int64).contiguous()
    ko = (C.c_float * 3)(*[float(v) for v in keepout]) if keepout is not None else None
    _lib.check(ops.lib.infgen_insert_cell_mask(
        _lib.ptr(p), _lib.ptr(h), _lib.ptr(st), _lib.ptr(na), _lib.ptr(av), _lib.ptr(sh), S, A, T, int(c), _lib.ptr(gx), G, rules, ko,
        float(clearance or 0.0), float(edge_clearance or 0.0), float(lane_dist or 0.0), sum(1 << int(t) for t in set(lane_types or ())),
        _lib.ptr(rc), _lib.ptr(nr), 0 if rc is None else int(rc.shape[1]), _lib.ptr(mp), _lib.ptr(mt), _lib.ptr(nm),
        0 if mp is None else int(mp.shape[1]), _lib.ptr(zn), _lib.ptr(nz), 0 if zn is None else int(zn.shape[1]), int(copies), 0, None,
        _lib.ptr(bits), W, _lib.ptr(count), _lib.ptr(live), None, 0, ops.stream), 'infgen_insert_cell_mask')
    return bits, count, live


@insert_cell_mask.register_fake
def _(pos, head, state, n_agents, av_index, shape, c, grid_xy, keepout=None, clearance=None, edge_clearance=None, records=None,
      n_records=None, lane_dist=None, lane_types=None, map_pos=None, map_type=None, n_map=None, zones=None, n_zones=None, copies=1):
    S = pos.shape[0]
    return (pos.new_empty(S, (grid_xy.shape[0] + 127) // 128 * 4, dtype=torch.int32), pos.new_empty(S, dtype=torch.int32),
            pos.new_empty(S, dtype=torch.int32))


def route_records(routes: torch.Tensor, n_points: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """the segment records of per-row routes ("route masks" of include/infgen_hip.h, ``infgen_route_records``): ``routes``
    (S0, A, P, 2) world-coordinate waypoints, 2 <= P <= 32, ``n_points`` (S0, A) -> records (S0, A, P - 1, 8), total (S0, A)"""
    if routes.dim() != 4 or routes.shape[3] != 2 or not 2 <= routes.shape[2] <= 32 or tuple(n_points.shape) != tuple(routes.shape[:2]):
        raise ValueError('route_records takes routes (S0, A, P, 2) with 2 <= P <= 32 and n_points (S0, A)')
    dev = routes.device
    ops = _ops(dev)
    S0, A, P = (int(v) for v in routes.shape[:3])
    rt, n = _f32(routes), n_points.to(dev, torch.int32).contiguous()
    rec, total = torch.zeros(S0, A, P - 1, 8, device=dev), torch.zeros(S0, A, device=dev)
    _lib.check(ops.lib.infgen_route_records(_lib.ptr(rt), _lib.ptr(n), S0, A, P, _lib.ptr(rec), _lib.ptr(total), ops.stream),
               'infgen_route_records')
    return rec, total


@torch.library.custom_op('infgen_hip::route_mask', mutates_args=())
def route_mask(pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, n_agents: torch.Tensor, type: torch.Tensor,
               shape: torch.Tensor, c: int, end_pose: torch.Tensor, records: torch.Tensor, total: torch.Tensor, copies: int = 1,
               corridor: float = 2.0, back: float = 0.5, pace: float = 0.0, finish: float = 1.0, types: Optional[List[int]] = None,
               mask_bits: Optional[torch.Tensor] = None, mask_row: Optional[torch.Tensor] = None,
               mask_type: Optional[List[int]] = None, first_new: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the allowed-token sets of one decode step from the rows' routes (route-following decoding; "route masks" of
    include/infgen_hip.h, ``infgen_route_mask``): the scene arrays and ``end_pose`` as for ``collision_mask``, ``records``
    (S / copies, A, P - 1, 8) and ``total`` (S / copies, A) from ``route_records``, ``types`` the (vehicle, pedestrian, cyclist)
    switch (None: vehicles and cyclists).  ``mask_bits`` / ``mask_row`` / ``mask_type``: the base sets (none: every token).  Returns
    the sets (S * A, token_size / 32) int32 words, the number of allowed tokens per row before the empty-set fallback (S * A,) and
    the progress (S * A, 4) = s0, d0, total, flag (1 ruled, 2 finished)."""
    if pos.dim() != 4 or pos.shape[3] != 2 or head.shape != pos.shape[:3] or state.shape != pos.shape[:3]:
        raise ValueError('route_mask takes pos (S, T, A, 2), head (S, T, A), state (S, T, A)')
    S, T, A = (int(v) for v in pos.shape[:3])
    if tuple(type.shape) != (S, A) or tuple(shape.shape) != (S, A, 3) or tuple(n_agents.shape) != (S,):
        raise ValueError('route_mask takes type (S, A), shape (S, A, 3), n_agents (S,)')
    if first_new is not None and tuple(first_new.shape) != (S,):
        raise ValueError('first_new must be (S,)')
    token_size = (int(end_pose.numel()) - 4) // 12
    if end_pose.dim() != 1 or token_size * 12 + 4 != end_pose.numel() or token_size % 32:
        raise ValueError('end_pose is the table of collision_end_poses (12 token_size + 4 floats, token_size a multiple of 32)')
    if copies < 1 or S % copies:
        raise ValueError('copies must be at least 1 and divide S')
    if records.dim() != 4 or records.shape[3] != 8 or tuple(records.shape[:2]) != (S // copies, A) or tuple(total.shape) != (S // copies, A):
        raise ValueError('route_mask takes records (S / copies, A, P - 1, 8) and total (S / copies, A)')
    types = [1, 0, 1] if types is None else [int(bool(v)) for v in types]
    if len(types) != 3:
        raise ValueError('types has three entries: vehicle, pedestrian, cyclist')
    dev = pos.device
    ops = _ops(dev)
    i32 = lambda t: None if t is None else t.to(dev, torch.int32).contiguous()
    ty = i32(type)
    tm, _keep_mask = _token_mask(mask_bits, mask_row, mask_type, ty.reshape(-1), S * A, token_size, dev)
    bits = torch.zeros(S * A, token_size // 32, device=dev, dtype=torch.int32)
    count = torch.zeros(S * A, device=dev, dtype=torch.int32)
    progress = torch.zeros(S * A, 4, device=dev)
    st, na, fn = i32(state), i32(n_agents), i32(first_new)
    p, h, sh, ep, rc, tt = _f32(pos), _f32(head), _f32(shape), _f32(end_pose), _f32(records), _f32(total)
    _lib.check(ops.lib.infgen_route_mask(_lib.ptr(p), _lib.ptr(h), _lib.ptr(st), _lib.ptr(na), _lib.ptr(fn), _lib.ptr(ty), _lib.ptr(sh),
                                         S, A, T, int(c), _lib.ptr(ep), token_size, _lib.ptr(rc), _lib.ptr(tt),
                                         int(records.shape[2]) + 1, int(copies), float(corridor), float(back), float(pace),
                                         float(finish), (C.c_int * 3)(*types), *tm[:4], _lib.ptr(bits), _lib.ptr(count),
                                         _lib.ptr(progress), ops.stream), 'infgen_route_mask')
    return bits, count, progress


@route_mask.register_fake
def _(pos, head, state, n_agents, type, shape, c, end_pose, records, total, copies=1, corridor=2.0, back=0.5, pace=0.0, finish=1.0,
      types=None, mask_bits=None, mask_row=None, mask_type=None, first_new=None):
    rows = pos.shape[0] * pos.shape[2]
    return (pos.new_empty(rows, (end_pose.shape[0] - 4) // 12 // 32, dtype=torch.int32), pos.new_empty(rows, dtype=torch.int32),
            pos.new_empty(rows, 4, dtype=torch.float32))


def signal_records(lines: torch.Tensor, n_lines: torch.Tensor) -> torch.Tensor:
    """the records of per-scene stop lines ("signal masks" of include/infgen_hip.h, ``infgen_signal_records``): ``lines`` (S0, K, 4) =
    (ax, ay, bx, by) world coordinates, 1 <= K <= 64, ``n_lines`` (S0,) -> records (S0, K, 8)"""
    if lines.dim() != 3 or lines.shape[2] != 4 or not 1 <= lines.shape[1] <= 64 or tuple(n_lines.shape) != tuple(lines.shape[:1]):
        raise ValueError('signal_records takes lines (S0, K, 4) with 1 <= K <= 64 and n_lines (S0,)')
    dev = lines.device
    ops = _ops(dev)
    S0, K = (int(v) for v in lines.shape[:2])
    ln, n = _f32(lines), n_lines.to(dev, torch.int32).contiguous()
    rec = torch.zeros(S0, K, 8, device=dev)
    _lib.check(ops.lib.infgen_signal_records(_lib.ptr(ln), _lib.ptr(n), S0, K, _lib.ptr(rec), ops.stream), 'infgen_signal_records')
    return rec


@torch.library.custom_op('infgen_hip::signal_mask', mutates_args=())
def signal_mask(pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, n_agents: torch.Tensor, type: torch.Tensor,
                shape: torch.Tensor, c: int, end_pose: torch.Tensor, records: torch.Tensor, phase: torch.Tensor, t: int,
                copies: int = 1, setback: float = 0.5, align: float = 0.5, types: Optional[List[int]] = None,
                mask_bits: Optional[torch.Tensor] = None, mask_row: Optional[torch.Tensor] = None,
                mask_type: Optional[List[int]] = None, first_new: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the allowed-token sets of one decode step from the scene's stop lines (signal-aware decoding; "signal masks" of
    include/infgen_hip.h, ``infgen_signal_mask``): the scene arrays and ``end_pose`` as for ``collision_mask``, ``records``
    (S / copies, K, 8) from ``signal_records``, ``phase`` (S / copies, n_phase, K) uint8 (non-zero: closed), ``t`` the decode step
    whose phase row t mod n_phase is read, ``types`` the (vehicle, pedestrian, cyclist) switch (None: vehicles and cyclists).
    ``mask_bits`` / ``mask_row`` / ``mask_type``: the base sets (none: every token).  Returns the sets (S * A, token_size / 32) int32
    words, the number of allowed tokens per row before the empty-set fallback (S * A,) and info (S * A, 4) = gap, line, flag, 0."""
    if pos.dim() != 4 or pos.shape[3] != 2 or head.shape != pos.shape[:3] or state.shape != pos.shape[:3]:
        raise ValueError('signal_mask takes pos (S, T, A, 2), head (S, T, A), state (S, T, A)')
    S, T, A = (int(v) for v in pos.shape[:3])
    if tuple(type.shape) != (S, A) or tuple(shape.shape) != (S, A, 3) or tuple(n_agents.shape) != (S,):
        raise ValueError('signal_mask takes type (S, A), shape (S, A, 3), n_agents (S,)')
    if first_new is not None and tuple(first_new.shape) != (S,):
        raise ValueError('first_new must be (S,)')
    token_size = (int(end_pose.numel()) - 4) // 12
    if end_pose.dim() != 1 or token_size * 12 + 4 != end_pose.numel() or token_size % 32:
        raise ValueError('end_pose is the table of collision_end_poses (12 token_size + 4 floats, token_size a multiple of 32)')
    if copies < 1 or S % copies:
        raise ValueError('copies must be at least 1 and divide S')
    if records.dim() != 3 or records.shape[2] != 8 or records.shape[0] != S // copies:
        raise ValueError('signal_mask takes records (S / copies, K, 8)')
    K = int(records.shape[1])
    if phase.dim() != 3 or phase.dtype != torch.uint8 or phase.shape[0] != S // copies or phase.shape[1] < 1 or phase.shape[2] != K:
        raise ValueError('signal_mask takes phase (S / copies, n_phase >= 1, K) uint8')
    types = [1, 0, 1] if types is None else [int(bool(v)) for v in types]
    if len(types) != 3:
        raise ValueError('types has three entries: vehicle, pedestrian, cyclist')
    dev = pos.device
    ops = _ops(dev)
    i32 = lambda x: None if x is None else x.to(dev, torch.int32).contiguous()
    ty = i32(type)
    tm, _keep_mask = _token_mask(mask_bits, mask_row, mask_type, ty.reshape(-1), S * A, token_size, dev)
    bits = torch.zeros(S * A, token_size // 32, device=dev, dtype=torch.int32)
    count = torch.zeros(S * A, device=dev, dtype=torch.int32)
    info = torch.zeros(S * A, 4, device=dev)
    st, na, fn = i32(state), i32(n_agents), i32(first_new)
    p, h, sh, ep, rc, ph = _f32(pos), _f32(head), _f32(shape), _f32(end_pose), _f32(records), phase.to(dev).contiguous()
    _lib.check(ops.lib.infgen_signal_mask(_lib.ptr(p), _lib.ptr(h), _lib.ptr(st), _lib.ptr(na), _lib.ptr(fn), _lib.ptr(ty), _lib.ptr(sh),
                                          S, A, T, int(c), _lib.ptr(ep), token_size, _lib.ptr(rc), _lib.ptr(ph), int(phase.shape[1]), K,
                                          int(t), int(copies), float(setback), float(align), (C.c_int * 3)(*types), *tm[:4],
                                          _lib.ptr(bits), _lib.ptr(count), _lib.ptr(info), ops.stream), 'infgen_signal_mask')
    return bits, count, info


@signal_mask.register_fake
def _(pos, head, state, n_agents, type, shape, c, end_pose, records, phase, t, copies=1, setback=0.5, align=0.5, types=None,
      mask_bits=None, mask_row=None, mask_type=None, first_new=None):
    rows = pos.shape[0] * pos.shape[2]
    return (pos.new_empty(rows, (end_pose.shape[0] - 4) // 12 // 32, dtype=torch.int32), pos.new_empty(rows, dtype=torch.int32),
            pos.new_empty(rows, 4, dtype=torch.float32))


@torch.library.custom_op('infgen_hip::step_score', mutates_args=())
def step_score(pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, n_agents: torch.Tensor, type: torch.Tensor,
               shape: torch.Tensor, c1: int, records: Optional[torch.Tensor] = None, n_records: Optional[torch.Tensor] = None,
               copies: int = 1, sweep: int = 1, road_margin: float = 0.0, types: Optional[List[int]] = None,
               dt: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """the step scores of stored column ``c1`` ("step scores" of include/infgen_hip.h, ``infgen_step_score``): the scene arrays as
    for ``road_mask``, ``records`` (S / copies, capacity, 8) and ``n_records`` (S / copies,) from ``road_records_from_map`` /
    ``_from_segments`` (None: no road table, ``n_offroad`` 0), ``types`` the (vehicle, pedestrian, cyclist) switch of the off-road
    term (None: vehicles and cyclists).  Returns score (S, 8) = n_live, n_overlap, min_sep, n_offroad, max_accel, max_yaw_rate, 0, 0
    and the rows' flag bytes (S, A) uint8: bit 0 live, bit 1 overlap, bit 2 off-road."""
    if pos.dim() != 4 or pos.shape[3] != 2 or tuple(head.shape) != tuple(pos.shape[:3]) or tuple(state.shape) != tuple(pos.shape[:3]):
        raise ValueError('step_score takes pos (S, T, A, 2), head (S, T, A), state (S, T, A)')
    S, T, A = (int(v) for v in pos.shape[:3])
    if tuple(type.shape) != (S, A) or tuple(shape.shape) != (S, A, 3) or tuple(n_agents.shape) != (S,):
        raise ValueError('step_score takes type (S, A), shape (S, A, 3), n_agents (S,)')
    if copies < 1 or S % copies:
        raise ValueError('copies must be at least 1 and divide S')
    if (records is None) != (n_records is None):
        raise ValueError('records and n_records come together')
    if records is not None and (records.dim() != 3 or records.shape[2] != 8 or records.shape[0] != S // copies
                                or tuple(n_records.shape) != (S // copies,)):
        raise ValueError('step_score takes records (S / copies, capacity, 8) and n_records (S / copies,)')
    types = [1, 0, 1] if types is None else [int(bool(v)) for v in types]
    if len(types) != 3:
        raise ValueError('types has three entries: vehicle, pedestrian, cyclist')
    dev = pos.device
    ops = _ops(dev)
    i32 = lambda t: None if t is None else t.to(dev, torch.int32).contiguous()
    st, na, ty, nr = i32(state), i32(n_agents), i32(type), i32(n_records)
    p, h, sh = _f32(pos), _f32(head), _f32(shape)
    rc = None if records is None else _f32(records)
    score = torch.zeros(S, 8, device=dev)
    row = torch.zeros(S, A, device=dev, dtype=torch.uint8)
    _lib.check(ops.lib.infgen_step_score(_lib.ptr(p), _lib.ptr(h), _lib.ptr(st), _lib.ptr(na), _lib.ptr(ty), _lib.ptr(sh), S, A, T,
                                         int(c1), _lib.ptr(rc), _lib.ptr(nr), 0 if records is None else int(records.shape[1]),
                                         int(copies), int(sweep), float(road_margin), (C.c_int * 3)(*types), float(dt),
                                         _lib.ptr(score), 8, _lib.ptr(row), ops.stream), 'infgen_step_score')
    return score, row


@step_score.register_fake
def _(pos, head, state, n_agents, type, shape, c1, records=None, n_records=None, copies=1, sweep=1, road_margin=0.0, types=None,
      dt=0.5):
    return pos.new_empty(pos.shape[0], 8, dtype=torch.float32), pos.new_empty(pos.shape[0], pos.shape[2], dtype=torch.uint8)


@torch.library.custom_op('infgen_hip::observe_rows', mutates_args=())
def observe_rows(pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, n_agents: torch.Tensor, type: torch.Tensor,
                 shape: torch.Tensor, c: int, dt: float, map_pos: Optional[torch.Tensor] = None,
                 map_orient: Optional[torch.Tensor] = None, map_type: Optional[torch.Tensor] = None,
                 n_map: Optional[torch.Tensor] = None, copies: int = 1, rows: Optional[torch.Tensor] = None, neighbors: int = 8,
                 radius: Optional[float] = None, map_tokens: int = 0, map_radius: Optional[float] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """the agent-frame observation of stored column ``c`` ("observations" of include/infgen_hip.h, ``infgen_observe_rows``): the
    scene arrays as for ``step_score``, the map as ``map_pos`` (S / copies, M, 2), ``map_orient`` (S / copies, M), ``map_type``
    (S / copies, M) and ``n_map`` (S / copies,) - all four or none -, ``rows`` (N,) int global row indices s * A + i (None: every
    row in order), ``radius`` / ``map_radius`` None or inf: no limit (an operator schema cannot spell an infinite default, so None
    stands for it).  Returns self_feat (N, 8), nbr_feat (N, neighbors, 10), nbr_index (N, neighbors) int32, nbr_count (N,) int32,
    map_feat (N, map_tokens, 6), map_index (N, map_tokens) int32, map_count (N,) int32."""
    if pos.dim() != 4 or pos.shape[3] != 2 or tuple(head.shape) != tuple(pos.shape[:3]) or tuple(state.shape) != tuple(pos.shape[:3]):
        raise ValueError('observe_rows takes pos (S, T, A, 2), head (S, T, A), state (S, T, A)')
    S, T, A = (int(v) for v in pos.shape[:3])
    if tuple(type.shape) != (S, A) or tuple(shape.shape) != (S, A, 3) or tuple(n_agents.shape) != (S,):
        raise ValueError('observe_rows takes type (S, A), shape (S, A, 3), n_agents (S,)')
    if copies < 1 or S % copies:
        raise ValueError('copies must be at least 1 and divide S')
    maps = (map_pos, map_orient, map_type, n_map)
    if any(m is None for m in maps) != all(m is None for m in maps):
        raise ValueError('map_pos, map_orient, map_type and n_map come together')
    if map_pos is not None and (map_pos.dim() != 3 or map_pos.shape[0] != S // copies or map_pos.shape[2] != 2 or map_pos.shape[1] < 1
                                or tuple(map_orient.shape) != tuple(map_pos.shape[:2]) or tuple(map_type.shape) != tuple(map_pos.shape[:2])
                                or tuple(n_map.shape) != (S // copies,)):
        raise ValueError('observe_rows takes map_pos (S / copies, M, 2), map_orient (S / copies, M), map_type (S / copies, M), n_map (S / copies,)')
    radius, map_radius = (float('inf') if r is None else float(r) for r in (radius, map_radius))
    observe.check_params(c, T, dt, neighbors, radius, map_tokens, map_radius, map_pos is not None)
    observe.check_rows(rows)
    dev = pos.device
    ops = _ops(dev)
    i32 = lambda t: None if t is None else t.to(dev, torch.int32).contiguous()
    f32 = lambda t: None if t is None else _f32(t)
    r = i32(rows)
    res = observe.outputs(S * A if r is None else int(r.numel()), int(neighbors), int(map_tokens), dev)
    observe.launch(ops.lib, ops.stream, _f32(pos), _f32(head), i32(state), i32(n_agents), i32(type), _f32(shape), c, dt, f32(map_pos),
                   f32(map_orient), None if map_type is None else map_type.to(dev, torch.int64).contiguous(), i32(n_map), copies, r,
                   neighbors, radius, map_tokens, map_radius, res)
    return tuple(res[k] for k in observe.KEYS)


@observe_rows.register_fake
def _(pos, head, state, n_agents, type, shape, c, dt, map_pos=None, map_orient=None, map_type=None, n_map=None, copies=1, rows=None,
      neighbors=8, radius=None, map_tokens=0, map_radius=None):
    N = pos.shape[0] * pos.shape[2] if rows is None else rows.shape[0]
    f, i = (lambda *s: pos.new_empty(*s, dtype=torch.float32)), (lambda *s: pos.new_empty(*s, dtype=torch.int32))
    return (f(N, observe.SELF), f(N, neighbors, observe.NBR), i(N, neighbors), i(N), f(N, map_tokens, observe.MAP), i(N, map_tokens), i(N))


@torch.library.custom_op('infgen_hip::idm_command', mutates_args=('cmd_pose',))
def idm_command(pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, n_agents: torch.Tensor, type: torch.Tensor,
                shape: torch.Tensor, ctl_row: torch.Tensor, c: int, records: torch.Tensor, total: torch.Tensor,
                cmd_pose: torch.Tensor, copies: int = 1, v_des: Optional[torch.Tensor] = None, dt: float = 0.5,
                v0: Optional[List[float]] = None, headway: float = 1.5, s_min: float = 2.0, a_max: float = 1.5, b_comf: float = 2.0,
                b_max: float = 6.0, lateral: float = 0.5, keep: float = 0.5, types: Optional[List[int]] = None,
                stop_at_end: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """the target poses of the rule-based controlled rows ("IDM commands" of include/infgen_hip.h, ``infgen_idm_command``): the
    scene arrays as for ``step_score``, ``ctl_row`` (S, A) bool / uint8 (the controlled rows), ``c >= 1`` the newest stored column,
    ``records`` (S / copies, A, P - 1, 8) and ``total`` (S / copies, A) from ``route_records``, ``v_des`` (S / copies, A) the rows'
    own desired speeds where > 0, ``v0`` the (vehicle, pedestrian, cyclist) desired speeds and ``types`` their switch (None: the
    defaults of ``controllers.check_idm``).  Writes (x, y, heading) of every ruled row into the caller's ``cmd_pose`` (S, A, 3),
    contiguous float32 - the other rows keep what they hold - and returns state (S * A, 8) = s0, e0, v, gap, acc, v1, s1, flag and
    lead (S * A,) int32 = j, -1 (none) or -2 (the route's end)."""
    if pos.dim() != 4 or pos.shape[3] != 2 or tuple(head.shape) != tuple(pos.shape[:3]) or tuple(state.shape) != tuple(pos.shape[:3]):
        raise ValueError('idm_command takes pos (S, T, A, 2), head (S, T, A), state (S, T, A)')
    S, T, A = (int(v) for v in pos.shape[:3])
    if tuple(type.shape) != (S, A) or tuple(shape.shape) != (S, A, 3) or tuple(n_agents.shape) != (S,) or tuple(ctl_row.shape) != (S, A):
        raise ValueError('idm_command takes type (S, A), shape (S, A, 3), n_agents (S,), ctl_row (S, A)')
    if copies < 1 or S % copies:
        raise ValueError('copies must be at least 1 and divide S')
    if not 1 <= int(c) < T:
        raise ValueError(f'idm_command: column {c} outside 1 .. {T - 1}')
    if records.dim() != 4 or records.shape[3] != 8 or tuple(records.shape[:2]) != (S // copies, A) or tuple(total.shape) != (S // copies, A):
        raise ValueError('idm_command takes records (S / copies, A, P - 1, 8) and total (S / copies, A)')
    if v_des is not None and tuple(v_des.shape) != (S // copies, A):
        raise ValueError('v_des must be (S / copies, A)')
    dev = pos.device
    if tuple(cmd_pose.shape) != (S, A, 3) or cmd_pose.dtype != torch.float32 or not cmd_pose.is_contiguous() or cmd_pose.device != dev:
        raise ValueError('cmd_pose is written in place: a contiguous float32 tensor (S, A, 3) on the scene\'s device')
    conf = dict(dt=dt, headway=headway, s_min=s_min, a_max=a_max, b_comf=b_comf, b_max=b_max, lateral=lateral, keep=keep,
                stop_at_end=bool(stop_at_end))
    if v0 is not None:
        conf['v0'] = list(v0)
    if types is not None:
        conf['types'] = [int(bool(v)) for v in types]
    conf = controllers.check_idm(conf)
    ops = _ops(dev)
    i32 = lambda t: t.to(dev, torch.int32).contiguous()
    out = controllers.idm_buffers(S, A, dev)
    controllers.launch(ops.lib, ops.stream, _f32(pos), _f32(head), i32(state), i32(n_agents), i32(type), _f32(shape),
                       ctl_row.to(dev, torch.uint8).contiguous(), c, _f32(records), _f32(total), copies,
                       None if v_des is None else _f32(v_des), conf, cmd_pose, out)
    return out['state'], out['lead']


@idm_command.register_fake
def _(pos, head, state, n_agents, type, shape, ctl_row, c, records, total, cmd_pose, copies=1, v_des=None, dt=0.5, v0=None, headway=1.5,
      s_min=2.0, a_max=1.5, b_comf=2.0, b_max=6.0, lateral=0.5, keep=0.5, types=None, stop_at_end=True):
    rows = pos.shape[0] * pos.shape[2]
    return pos.new_empty(rows, 8, dtype=torch.float32), pos.new_empty(rows, dtype=torch.int32)


@torch.library.custom_op('infgen_hip::map_token_head', mutates_args=())
def map_token_head(x: torch.Tensor, rows: torch.Tensor, pack: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """the map encoder's token_predict_head and its top-10 (map_decoder.py:119-121) on rows ``rows`` of ``x`` (N, 128): raw logits
    (n, 1024) and the indices of the 10 most probable tokens (n, 10) int64, descending; ``pack`` = packing.pack_mlp_layer"""
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= x.shape[0]):
        raise IndexError(f'map_token_head: rows must index the {x.shape[0]} rows of x')
    if x.dim() != 2 or x.shape[1] != D or pack.numel() < 16768 + 129 * 1024:
        raise ValueError('map_token_head takes x (N, 128) and the MLPLayer pack of a 1024-token head')
    return _ops(x.device).map_token_head(_f32(x), rows.to(x.device, torch.int32).contiguous(), _f32(pack))


@map_token_head.register_fake
def _(x, rows, pack):
    n = rows.shape[0]
    return x.new_empty(n, 1024, dtype=torch.float32), x.new_empty(n, 10, dtype=torch.int64)


@torch.library.custom_op('infgen_hip::mlp_layer', mutates_args=())
def mlp_layer(x: torch.Tensor, pack: torch.Tensor, n_out: int) -> torch.Tensor:
    """MLPLayer.forward (layers.py:195-215): Linear - LayerNorm - ReLU - Linear"""
    ops = _ops(x.device)
    if x.shape[0] == 0:
        return x.new_empty(0, n_out, dtype=torch.float32)
    return ops.mlp_layer(_f32(x), _f32(pack), x.shape[1], int(n_out))


@mlp_layer.register_fake
def _(x, pack, n_out):
    return x.new_empty(x.shape[0], n_out, dtype=torch.float32)


@torch.library.custom_op('infgen_hip::mlp_embedding', mutates_args=())
def mlp_embedding(x: torch.Tensor, pack: torch.Tensor) -> torch.Tensor:
    """MLPEmbedding.forward (layers.py:163-192)"""
    ops = _ops(x.device)
    if x.shape[0] == 0:
        return x.new_empty(0, D, dtype=torch.float32)
    return ops.mlp_embedding(_f32(x), _f32(pack), x.shape[1])


@mlp_embedding.register_fake
def _(x, pack):
    return x.new_empty(x.shape[0], D, dtype=torch.float32)


@torch.library.custom_op('infgen_hip::integrate_tokenise', mutates_args=())
def integrate_tokenise(token: torch.Tensor, state: torch.Tensor, agent_type: torch.Tensor, pos: torch.Tensor, head: torch.Tensor,
                       n_agents: torch.Tensor, ego: torch.Tensor, vocab: torch.Tensor, grid_xy: torch.Tensor
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """token -> trajectory -> next pose -> grid cell for dense batches (reference agent_decoder.py:2175-2239,
    attr_tokenizer.py:77-89): ``token`` / ``state`` / ``agent_type`` (S, A) int, ``pos`` (S, A, 2), ``head`` (S, A) the current
    pose, ``n_agents`` / ``ego`` (S,), ``vocab`` (3, token_size, 6, 4, 2), ``grid_xy`` (G, 2).  ``state`` is the state head's
    class index (2 -> exit; the ego is forced valid).  Returns the next pose ``pos'`` (S, A, 2), ``head'`` (S, A) (zeros for
    invalid rows), the five intermediate poses ``pred_traj`` (S, A, 5, 2) / ``pred_head`` (S, A, 5), the cell of the new position in
    the ego's new frame ``grid`` (S, A) (-1 invalid) and the stored ``state'`` (S, A).  One launch of ``infgen_integrate``."""
    dev = pos.device
    ops = _ops(dev)
    S, A = token.shape
    A_cap = max(32, (A + 31) // 32 * 32)
    if A_cap > ops.lib.infgen_layout_query(_lib.Q_MAX_AGENTS):
        raise _lib.InfgenHipError('integrate_tokenise: more rows per scene than the layout holds')
    i32 = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.int32)
    T = 3
    P = torch.zeros(S, T, A_cap, 2, device=dev); H = torch.zeros(S, T, A_cap, device=dev)
    ST, TK, GR = i32(S, T, A_cap), i32(S, T, A_cap), i32(S, T, A_cap)
    IM = torch.ones(S, T, A_cap, device=dev, dtype=torch.uint8); CF = torch.ones_like(IM); TM = torch.ones_like(IM)
    P[:, 1, :A] = pos.float(); H[:, 1, :A] = head.float()
    ty, nt, ns = i32(S, A_cap), i32(S, A_cap), i32(S, A_cap)
    ty[:, :A] = agent_type.int(); nt[:, :A] = token.int(); ns[:, :A] = state.int()
    bos = i32(S, A_cap)
    na, av = n_agents.to(dev).int().contiguous(), ego.to(dev).int().contiguous()
    traj, phead, pstate = torch.zeros(S, A_cap, 5, 2, device=dev), torch.zeros(S, A_cap, 5, device=dev), torch.zeros(S, A_cap, 5, device=dev)
    voc, gxy = _f32(vocab), _f32(grid_xy)
    c = _lib.Rollout()
    Pp = _lib.ptr
    c.S, c.A_cap, c.T, c.M_cap, c.W, c.ring, c.R = S, A_cap, T, 32, 1, 2, 5
    c.token_size, c.grid_size, c.num_layers = int(voc.shape[1]), int(gxy.shape[0]), 1
    c.n_agents, c.n_map, c.av_index = Pp(na), Pp(i32(S)), Pp(av)
    c.pos, c.head, c.state, c.token, c.grid = Pp(P), Pp(H), Pp(ST), Pp(TK), Pp(GR)
    c.tmask, c.imask, c.catflag, c.type, c.bos = Pp(TM), Pp(IM), Pp(CF), Pp(ty), Pp(bos)
    c.next_token, c.next_state = Pp(nt.view(-1)), Pp(ns.view(-1))
    c.vocab, c.grid_xy = Pp(voc), Pp(gxy)
    c.pred_traj, c.pred_head, c.pred_state = Pp(traj), Pp(phead), Pp(pstate)
    if S and A:
        _lib.check(ops.lib.infgen_integrate(C.byref(c), 0, ops.stream), 'infgen_integrate')
    return (P[:, 2, :A].contiguous(), H[:, 2, :A].contiguous(), traj[:, :A].contiguous(), phead[:, :A].contiguous(),
            GR[:, 2, :A].contiguous(), ST[:, 2, :A].contiguous())


@integrate_tokenise.register_fake
def _(token, state, agent_type, pos, head, n_agents, ego, vocab, grid_xy):
    S, A = token.shape
    f = lambda *shape: pos.new_empty(*shape, dtype=torch.float32)
    i = lambda *shape: pos.new_empty(*shape, dtype=torch.int32)
    return f(S, A, 2), f(S, A), f(S, A, 5, 2), f(S, A, 5), i(S, A), i(S, A)


@torch.library.custom_op('infgen_hip::decode_step',
                         mutates_args=('pos', 'head', 'state', 'token', 'grid', 'x', 'next_token', 'next_state'))
def decode_step(ctx: torch.Tensor, t: int, pos: torch.Tensor, head: torch.Tensor, state: torch.Tensor, token: torch.Tensor,
                grid: torch.Tensor, x: torch.Tensor, next_token: torch.Tensor, next_state: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """one decode step over a persistent state block (reference agent_decoder.py:1740-2301 without the
    insertion sub-loop): edge sets of column 1 + t, the 18 sublayers, heads, token -> pose -> grid cell, raw feature of the new
    column - ``infgen_decode_step``.  ``ctx``: the bytes of the ``InfgenRollout`` block (include/infgen_hip.h) as a uint8 CPU
    tensor (``RolloutEngine.ctx_tensor()``); the arrays the block points to that a step writes are passed (and declared
    mutated) so that a tracer sees the data flow: ``pos`` / ``head`` / ``state`` / ``token`` / ``grid`` [S][T][A_cap], the residual
    stream ``x`` [rows][128] and the heads' outputs ``next_token`` / ``next_state`` [rows], copies of which are returned."""
    ops = _ops(pos.device)
    blk = _lib.Rollout.from_buffer_copy(ctx.numpy().tobytes())
    for name, ten in (('pos', pos), ('head', head), ('state', state), ('token', token), ('grid', grid), ('X', x),
                      ('next_token', next_token), ('next_state', next_state)):
        if int(getattr(blk, name) or 0) != ten.data_ptr():
            raise _lib.InfgenHipError(f'decode_step: `{name}` is not the array the state block points to')
    _lib.check(ops.lib.infgen_decode_step(C.byref(blk), int(t), ops.stream), 'infgen_decode_step')
    return next_token.clone(), next_state.clone()


@decode_step.register_fake
def _(ctx, t, pos, head, state, token, grid, x, next_token, next_state):
    return torch.empty_like(next_token), torch.empty_like(next_state)


@torch.library.custom_op('infgen_hip::command_rows', mutates_args=('teacher_token', 'teacher_state'))
def command_rows(ctx: torch.Tensor, t: int, teacher_token: torch.Tensor, teacher_state: torch.Tensor,
                 cmd_token: Optional[torch.Tensor] = None, cmd_pose: Optional[torch.Tensor] = None,
                 cmd_mask: Optional[torch.Tensor] = None, shape: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a closed-loop session's commands of decode step ``t`` -> column 2 + t of the plan the flagged rows of the state block
    follow (``infgen_command_rows``; call it in front of ``decode_step(ctx, t, ...)``).  ``ctx`` as in ``decode_step``;
    ``teacher_token`` / ``teacher_state`` [S][T][A_cap]: the block's plan arrays (declared mutated; with pose arrays in the block
    the commanded pose is written there too).  One of ``cmd_token`` [S][A_cap] int (token ids) and ``cmd_pose`` [S][A_cap][3]
    (x, y, heading; needs ``shape`` [S][A_cap][3] = length, width, height: the nearest motion token of the row's vocabulary is
    matched on the device); ``cmd_mask`` [S][A_cap] (optional): 0 = the row leaves the scene.  Returns the matching cost [S][A_cap]
    (0 for token commands and for rows that are not commanded).  No host read."""
    ops = _ops(teacher_token.device)
    dev = teacher_token.device
    blk = _lib.Rollout.from_buffer_copy(ctx.numpy().tobytes())
    for name, ten in (('teacher_token', teacher_token), ('teacher_state', teacher_state)):
        if int(getattr(blk, name) or 0) != ten.data_ptr():
            raise _lib.InfgenHipError(f'command_rows: `{name}` is not the array the state block points to')
    if (cmd_token is None) == (cmd_pose is None):
        raise ValueError('command_rows takes cmd_token or cmd_pose, one of them')
    S, A_cap = int(blk.S), int(blk.A_cap)

    def arr(x, dtype, tail=()):
        if x is None:
            return None
        if tuple(x.shape) != (S, A_cap) + tail:
            raise ValueError(f'command_rows: expected shape {(S, A_cap) + tail}, got {tuple(x.shape)}')
        return x.to(dev, dtype).contiguous()
    tok, pose = arr(cmd_token, torch.int32), arr(cmd_pose, torch.float32, (3,))
    msk, shp = arr(cmd_mask, torch.uint8), arr(shape, torch.float32, (3,))
    cost = torch.zeros(S, A_cap, device=dev)
    _lib.check(ops.lib.infgen_command_rows(C.byref(blk), int(t), 0 if tok is not None else 1, _lib.ptr(tok), _lib.ptr(pose),
                                           _lib.ptr(msk), _lib.ptr(shp), _lib.ptr(cost), ops.stream), 'infgen_command_rows')
    return cost


@command_rows.register_fake
def _(ctx, t, teacher_token, teacher_state, cmd_token=None, cmd_pose=None, cmd_mask=None, shape=None):
    return teacher_token.new_empty(teacher_token.shape[0], teacher_token.shape[2], dtype=torch.float32)


@torch.library.custom_op('infgen_hip::branch_scenes', mutates_args=())
def branch_scenes(ctx: torch.Tensor, t: int, parent: torch.Tensor) -> torch.Tensor:
    """branching rollouts (``infgen_branch_scenes``; "branching" of include/infgen_hip.h): every slot s of the state block with
    ``parent[s] != s`` becomes a clone of slot ``parent[s]`` as of the boundary in front of decode step ``t``.  ``ctx`` as in
    ``decode_step``; ``parent`` [S] or [S0, copies] int device tensor of global slot indices (same copy group, sources fixed
    points).  The ~30 arrays the block points to are edited in place (not declared: the block owns them); returns the number of
    entries that broke the contract and were treated as the identity, (1,) int32.  No host read."""
    if not parent.is_cuda:
        raise _lib.InfgenHipError('infgen_hip ops need cuda tensors: the HIP path has no CPU fallback')
    if parent.is_floating_point() or parent.dtype == torch.bool:
        raise ValueError('branch_scenes: parent holds integer slot indices')
    ops = _ops(parent.device)
    blk = _lib.Rollout.from_buffer_copy(ctx.numpy().tobytes())
    if parent.numel() != int(blk.S):
        raise ValueError(f'branch_scenes: parent must hold one entry per scene slot ({int(blk.S)})')
    p = parent.to(torch.int32).contiguous().view(-1)
    bad = torch.zeros(1, device=parent.device, dtype=torch.int32)
    _lib.check(ops.lib.infgen_branch_scenes(C.byref(blk), int(t), _lib.ptr(p), _lib.ptr(bad), ops.stream), 'infgen_branch_scenes')
    return bad


@branch_scenes.register_fake
def _(ctx, t, parent):
    return parent.new_empty(1, dtype=torch.int32)


def _snapshot_args(what, blk, sel, snap, head):
    if not (sel.is_cuda and snap.is_cuda and head.is_cuda):
        raise _lib.InfgenHipError('infgen_hip ops need cuda tensors: the HIP path has no CPU fallback')
    if sel.is_floating_point() or sel.dtype == torch.bool:
        raise ValueError(f'{what}: slot and entry indices are integers')
    if snap.dtype != torch.uint8 or snap.dim() != 2 or not snap.is_contiguous():
        raise ValueError(f'{what}: snap is a contiguous uint8 tensor [entries, stride]')
    if head.dtype != torch.int32 or tuple(head.shape) != (snap.shape[0], 4) or not head.is_contiguous():
        raise ValueError(f'{what}: head is a contiguous int32 tensor [entries, 4]')
    return sel.to(torch.int32).contiguous().view(-1)


@torch.library.custom_op('infgen_hip::snapshot_scenes', mutates_args=('snap', 'head'))
def snapshot_scenes(ctx: torch.Tensor, t: int, slots: torch.Tensor, snap: torch.Tensor, head: torch.Tensor) -> torch.Tensor:
    """snapshots (``infgen_snapshot_scenes``; "snapshots" of include/infgen_hip.h): entry e of ``snap`` (uint8 [n, stride], stride at
    least ``infgen_snapshot_bytes``) receives the decode state of slot ``slots[e]`` of the state block as of the boundary in front
    of decode step ``t``, and ``head`` (int32 [n, 4]) its {slot, group, t, valid}.  ``ctx`` as in ``decode_step``; ``slots`` [n] int
    device tensor.  The block's arrays are not written.  Returns the number of slots out of range, (1,) int32.  No host read."""
    ops = _ops(snap.device)
    blk = _lib.Rollout.from_buffer_copy(ctx.numpy().tobytes())
    s = _snapshot_args('snapshot_scenes', blk, slots, snap, head)
    if s.numel() != snap.shape[0]:
        raise ValueError(f'snapshot_scenes: one slot per entry ({int(snap.shape[0])})')
    bad = torch.zeros(1, device=snap.device, dtype=torch.int32)
    _lib.check(ops.lib.infgen_snapshot_scenes(C.byref(blk), int(t), _lib.ptr(s), int(s.numel()), _lib.ptr(snap), int(snap.shape[1]),
                                              _lib.ptr(head), _lib.ptr(bad), ops.stream), 'infgen_snapshot_scenes')
    return bad


@snapshot_scenes.register_fake
def _(ctx, t, slots, snap, head):
    return slots.new_empty(1, dtype=torch.int32)


@torch.library.custom_op('infgen_hip::restore_scenes', mutates_args=())
def restore_scenes(ctx: torch.Tensor, t: int, index: torch.Tensor, snap: torch.Tensor, head: torch.Tensor) -> torch.Tensor:
    """snapshots (``infgen_restore_scenes``): slot s of the state block receives entry ``index[s]`` of ``snap`` (-1: keep), where that
    entry's ``head`` row says valid, step ``t`` and slot s's copy group.  ``index`` [S] or [S0, copies] int device tensor.  The ~30
    arrays the block points to are edited in place (not declared: the block owns them); returns the number of entries that were
    refused and read as -1, (1,) int32.  No host read."""
    ops = _ops(snap.device)
    blk = _lib.Rollout.from_buffer_copy(ctx.numpy().tobytes())
    x = _snapshot_args('restore_scenes', blk, index, snap, head)
    if x.numel() != int(blk.S):
        raise ValueError(f'restore_scenes: index must hold one entry per scene slot ({int(blk.S)})')
    bad = torch.zeros(1, device=snap.device, dtype=torch.int32)
    _lib.check(ops.lib.infgen_restore_scenes(C.byref(blk), int(t), _lib.ptr(x), _lib.ptr(snap), int(snap.shape[1]), _lib.ptr(head),
                                             int(snap.shape[0]), _lib.ptr(bad), ops.stream), 'infgen_restore_scenes')
    return bad


@restore_scenes.register_fake
def _(ctx, t, index, snap, head):
    return index.new_empty(1, dtype=torch.int32)


@torch.library.custom_op('infgen_hip::bundle_scores', mutates_args=())
def bundle_scores(valid: torch.Tensor, collision: torch.Tensor, linear_speed: torch.Tensor, linear_acceleration: torch.Tensor,
                  angular_speed: torch.Tensor, angular_acceleration: torch.Tensor, distance_to_nearest_object: torch.Tensor,
                  time_to_collision: torch.Tensor, distance_placement: torch.Tensor, distance_removement: torch.Tensor,
                  num_placement: torch.Tensor, num_removement: torch.Tensor, n_rows: torch.Tensor, table: torch.Tensor,
                  n_scenario: int, size: int = 80, step: int = 5, shift: int = 5
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """the realism scores of all rollouts of all scenarios of a batch (reference compute_scenario_metrics_for_bundle,
    infgen/metrics/compute_metrics.py:891-1103) - ``infgen_bundle_scores``: per-object arrays (B, N, T) [placement distances
    (B, N, T2), counts (B, T2)] with B = n_scenario * n_rollout bundles padded to N rows, ``n_rows`` (B,) real rows, ``table``
    from ``infgen_amd.metrics.pack_score_table`` -> scalars (n_scenario, 13), per-window values (n_scenario, 12, W),
    per-rollout count likelihoods (B, 2, W), counters (3,) int32"""
    dev = valid.device
    ops = _ops(dev)
    B, N, T = valid.shape
    T2 = distance_placement.shape[-1]
    W = (T - size) // step + 1
    u8 = lambda t: t.contiguous().to(torch.uint8)
    byt = [u8(valid), u8(collision)]
    flt = [_f32(t) for t in (linear_speed, linear_acceleration, angular_speed, angular_acceleration,
                             distance_to_nearest_object, time_to_collision, distance_placement, distance_removement)]
    cnt = [t.contiguous().long() for t in (num_placement, num_removement)]
    rows, tab = n_rows.contiguous().to(torch.int32), _f32(table)
    scal = torch.empty(n_scenario, 13, device=dev)
    lng = torch.empty(n_scenario, 12, max(W, 0), device=dev)
    per = torch.empty(B, 2, max(W, 0), device=dev)
    counters = torch.zeros(3, device=dev, dtype=torch.int32)
    P = _lib.ptr
    _lib.check(ops.lib.infgen_bundle_scores(*(P(t) for t in byt + flt + cnt), P(rows), P(tab), int(n_scenario),
                                            B // max(int(n_scenario), 1), N, T, T, T2, T2, T2, int(size), int(step), int(shift),
                                            P(scal), P(lng), P(per), P(counters), ops.stream), 'infgen_bundle_scores')
    return scal, lng, per, counters


@bundle_scores.register_fake
def _(valid, collision, linear_speed, linear_acceleration, angular_speed, angular_acceleration, distance_to_nearest_object,
      time_to_collision, distance_placement, distance_removement, num_placement, num_removement, n_rows, table, n_scenario,
      size=80, step=5, shift=5):
    W = (valid.shape[2] - size) // step + 1
    f = lambda *shape: valid.new_empty(*shape, dtype=torch.float32)
    return f(n_scenario, 13), f(n_scenario, 12, W), f(valid.shape[0], 2, W), valid.new_empty(3, dtype=torch.int32)


@torch.library.custom_op('infgen_hip::select_modes', mutates_args=())
def select_modes(traj: torch.Tensor, k: int = 6, dist_thresh: float = 2.5, scores: Optional[torch.Tensor] = None,
                 valid: Optional[torch.Tensor] = None, t_goal: int = -1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """K modes per row out of N candidate trajectories (the reference's batch_nms / new_batch_nms; ``infgen_select_modes``,
    "modes" of include/infgen_hip.h): ``traj`` (B, N, T, F) read in place, ``scores`` (B, N) >= 0 or None (the goals' density),
    ``valid`` (B, N) or None -> mode_traj (B, k, T, F), mode_score (B, k), mode_idx (B, k) int32 (-1: fewer than k valid candidates)"""
    from . import modes
    return modes.select_modes(traj, k=int(k), dist_thresh=float(dist_thresh), scores=scores, valid=valid, t_goal=int(t_goal))


@select_modes.register_fake
def _(traj, k=6, dist_thresh=2.5, scores=None, valid=None, t_goal=-1):
    lead = tuple(traj.shape[:-3])
    return (traj.new_empty(lead + (k,) + tuple(traj.shape[-2:]), dtype=torch.float32), traj.new_empty(lead + (k,), dtype=torch.float32),
            traj.new_empty(lead + (k,), dtype=torch.int32))
