"""Mirror of the reference's ``infgen/utils/metrics.py`` for the validation step, on the device and without torchmetrics:
``TokenCls``, ``minADE``, ``minFDE``, ``AverageMeter``, ``StateAccuracy``, ``GridOverlapRate``, ``NumInsertAccuracy`` with the
reference's constructor arguments, ``update`` signatures, ``compute`` keys and ``__repr__`` text, plus ``masked_cross_entropy`` -
the ``pred[mask]`` + ``nn.CrossEntropyLoss`` of the open-loop branch (infgen/model/infgen.py:644, :655) without the boolean gather.

Every class follows ``infgen_amd.metrics.LongMetric``: ``update`` / ``compute`` / ``reset`` and ``state()`` / ``merge()`` for the sum
reduction across ranks (``dist_reduce_fx='sum'`` of every state in the reference).  The state of an object is ONE device buffer of
8-byte slots (int64 counters, float64 sums); ``update`` launches the kernels of infgen_amd/csrc/val_metrics.hip on the current
stream and returns - nothing is read back; ``compute`` returns device tensors, the only host copy is the caller's.  Floating sums
are accumulated in float64 in a fixed order (bitwise reproducible), so ``minADE`` / ``minFDE`` / ``AverageMeter`` / the loss
return float64 where the reference returns float32.  The product path has no host implementation: a CPU tensor raises
``InfgenHipError``.

Index tensors may be int32 or int64, masks bool or uint8 - what ``InfGenDecoder.inference`` / ``forward`` / ``fetch_enterings``
deliver - and are read in place (a view with a unit inner stride included); any other mask dtype is converted to uint8 first.

``minMultiADE`` / ``minMultiFDE`` (:339-427; nothing in the reference's validation constructs them, a user of many rollouts per
scene does) run ``valid_filter`` and the plain ``topk`` inside their one kernel, ``k_multi_traj_error``; their ``update`` takes the
K modes ``infgen_amd.modes`` selects - the reference's ``batch_nms`` / ``new_batch_nms`` live there, not in this module.

Left out on purpose:
  * ``batch_nms_token`` and ``batch_nms(mode='speed')``: ``infgen_amd.modes`` raises NotImplementedError naming them.
  * the joint / ``ptr`` variants of ``topk`` (:58-67) and ``topkind``: nothing in the reference calls them.
  * the ``val_insert`` branch (infgen/model/infgen.py:688-700): it calls ``NumInsertAccuracy.update`` with keyword names the method
    does not have and the attribute is commented out at :144 - the class is mirrored, the branch is not.
  * ``CustomCrossEntropyLoss``: ``masked_cross_entropy(label_smoothing=...)`` covers it.
"""
from typing import Dict, Optional

import torch

from .. import _lib
from .._lib import InfgenHipError

__all__ = ['minADE', 'minFDE', 'TokenCls', 'StateAccuracy', 'GridOverlapRate']


def _dev(t, name: str) -> torch.device:
    if not torch.is_tensor(t) or t.device.type != 'cuda':
        where = t.device if torch.is_tensor(t) else type(t).__name__
        raise InfgenHipError(f'{name} must be a GPU tensor (got {where}): the validation metrics run on the device only, '
                             f'there is no host implementation')
    return t.device


def _rows(t: torch.Tensor, name: str, dev: torch.device):
    """an index matrix [N, T] read in place -> (tensor kept alive, is64, row stride)"""
    if _dev(t, name) != dev:
        raise InfgenHipError(f'{name} is on {t.device}, expected {dev}')
    if t.dtype not in (torch.int32, torch.int64):
        raise InfgenHipError(f'{name} must be int32 or int64, not {t.dtype}')
    if t.dim() != 2:
        raise InfgenHipError(f'{name} must have two dimensions, not {tuple(t.shape)}')
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if ld < t.shape[1]:
        t, ld = t.contiguous(), t.shape[1]
    return t, int(t.dtype == torch.int64), int(ld)


def _bytes(t: torch.Tensor, name: str, dev: torch.device) -> torch.Tensor:
    """a mask as bytes: bool is reinterpreted, uint8 taken as it is, anything else converted"""
    if _dev(t, name) != dev:
        raise InfgenHipError(f'{name} is on {t.device}, expected {dev}')
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t if t.dtype == torch.uint8 else t.to(torch.uint8)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _DeviceMetric:
    """state = one device buffer of ``_slots`` 8-byte slots; ``_float_slots`` of them hold float64 sums, the rest int64 counters"""
    _slots = 0
    _float_slots = ()

    def __init__(self, **kwargs) -> None:
        self._buf: Optional[torch.Tensor] = None
        self._scratch: Optional[torch.Tensor] = None

    def _state_buf(self, dev: Optional[torch.device] = None) -> torch.Tensor:
        if self._buf is None:
            if dev is None:
                if not torch.cuda.is_available():
                    raise InfgenHipError(f'{type(self).__name__} needs a GPU (no host implementation)')
                dev = torch.device('cuda', torch.cuda.current_device())
            self._buf = torch.zeros(self._slots, dtype=torch.int64, device=dev)
        elif dev is not None and self._buf.device != dev:
            raise InfgenHipError(f'{type(self).__name__} accumulates on {self._buf.device}; update() got tensors on {dev}')
        return self._buf

    def _scratch_buf(self, dev) -> torch.Tensor:
        if self._scratch is None or self._scratch.device != dev:
            self._scratch = torch.empty(_lib.VM_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
        return self._scratch

    def reset(self) -> None:
        if self._buf is not None:
            self._buf.zero_()

    def state(self) -> Dict:
        """a copy of the accumulated state (a device tensor; safe to merge elsewhere)"""
        return dict(buf=self._state_buf().clone())

    def merge(self, other_state: Dict) -> None:
        """add another object's / rank's state (dist_reduce_fx 'sum')"""
        buf = self._state_buf()
        other = other_state['buf'].to(buf.device)
        if other.shape != buf.shape:
            raise InfgenHipError(f'{type(self).__name__}.merge: state of {tuple(other.shape)} slots, expected {tuple(buf.shape)}')
        fl = list(self._float_slots)
        if fl:
            f_new = buf.view(torch.float64)[fl] + other.view(torch.float64)[fl]
        buf += other
        if fl:
            buf.view(torch.float64)[fl] = f_new


class TokenCls(_DeviceMetric):
    """reference :316-336"""
    _slots = 2

    def __init__(self, max_guesses: int = 6, **kwargs) -> None:
        super().__init__(**kwargs)
        self.max_guesses = max_guesses

    def update(self, pred: torch.Tensor, target: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> None:
        dev = _dev(pred, 'pred')
        if valid_mask is None:
            raise InfgenHipError('TokenCls.update needs valid_mask (the reference multiplies by it)')
        if pred.dim() != 2:
            raise InfgenHipError(f'pred must be [rows, guesses], not {tuple(pred.shape)}')
        p, p64, ldp = _rows(pred, 'pred', dev)
        t, t64, _ = _rows(target.reshape(-1, 1), 'target', dev)
        m = _bytes(valid_mask, 'valid_mask', dev).reshape(-1)
        R = p.shape[0]
        if t.shape[0] != R or m.shape[0] != R:
            raise InfgenHipError(f'pred has {R} rows, target {t.shape[0]}, valid_mask {m.shape[0]}')
        t, m = t.contiguous(), m.contiguous()
        n_guess = max(0, min(int(self.max_guesses), p.shape[1]))
        _lib.check(_lib.load().infgen_token_cls(p.data_ptr(), p64, max(ldp, n_guess), n_guess, t.data_ptr(), t64, m.data_ptr(), R,
                                                self._state_buf(dev).data_ptr(), _stream(dev)), 'infgen_token_cls')

    def compute(self) -> torch.Tensor:
        b = self._state_buf()
        return b[0] / b[1]


class _TrajMetric(_DeviceMetric):
    _slots = 2
    _float_slots = (0,)

    def __init__(self, max_guesses: int = 6, **kwargs) -> None:
        super().__init__(**kwargs)
        self.max_guesses = max_guesses
        self.eval_timestep = 70          # (the kernel's constant: E = min(70, T))

    def compute(self) -> torch.Tensor:
        b = self._state_buf()
        return b.view(torch.float64)[0] / b[1]


def update_traj_metrics(ade: Optional['minADE'], fde: Optional['minFDE'], pred: torch.Tensor, target: torch.Tensor,
                        valid_mask: torch.Tensor) -> None:
    """``minADE.update`` and ``minFDE.update`` of the same arguments in ONE pass over pred / target [N, T, 2], valid_mask [N, T]"""
    dev = _dev(pred, 'pred')
    _dev(target, 'target')
    if valid_mask is None:
        raise InfgenHipError('minADE / minFDE need valid_mask')
    if pred.dim() != 3 or pred.shape[-1] != 2 or target.shape != pred.shape or tuple(valid_mask.shape) != tuple(pred.shape[:2]):
        raise InfgenHipError(f'need pred / target [N, T, 2] and valid_mask [N, T], got {tuple(pred.shape)}, {tuple(target.shape)}, '
                             f'{tuple(valid_mask.shape)}')
    p, q = pred.to(torch.float32).contiguous(), target.to(torch.float32).contiguous()
    v = _bytes(valid_mask, 'valid_mask', dev).contiguous()
    owner = ade if ade is not None else fde
    _lib.check(_lib.load().infgen_traj_error(p.data_ptr(), q.data_ptr(), v.data_ptr(), p.shape[0], p.shape[1],
                                             ade._state_buf(dev).data_ptr() if ade is not None else None,
                                             fde._state_buf(dev).data_ptr() if fde is not None else None,
                                             owner._scratch_buf(dev).data_ptr(), _stream(dev)), 'infgen_traj_error')


class minFDE(_TrajMetric):
    """reference :367-390: the single column min(70, T) - 2, weighted by its valid flag"""

    def update(self, pred: torch.Tensor, target: torch.Tensor, prob: Optional[torch.Tensor] = None,
               valid_mask: Optional[torch.Tensor] = None, keep_invalid_final_step: bool = True) -> None:
        update_traj_metrics(None, self, pred, target, valid_mask)


class minADE(_TrajMetric):
    """reference :430-467: columns below min(70, T), each row divided by T, rows with any valid column counted"""

    def update(self, pred: torch.Tensor, target: torch.Tensor, prob: Optional[torch.Tensor] = None,
               valid_mask: Optional[torch.Tensor] = None, keep_invalid_final_step: bool = True,
               min_criterion: str = 'ADE') -> None:
        update_traj_metrics(self, None, pred, target, valid_mask)


_MIN_CRITERIA = {'FDE': 0, 'ADE': 1}


def update_multi_traj_metrics(ade: Optional['minMultiADE'], fde: Optional['minMultiFDE'], pred: torch.Tensor, target: torch.Tensor,
                              prob: Optional[torch.Tensor] = None, valid_mask: Optional[torch.Tensor] = None,
                              keep_invalid_final_step: bool = True, min_criterion: str = 'FDE') -> None:
    """``minMultiADE.update`` and ``minMultiFDE.update`` of the same arguments in ONE pass over pred [N, M, T, 2], target [N, T, 2],
    prob [N, M] or None, valid_mask [N, T] or None (all valid); ``max_guesses`` is the ADE object's (the FDE object's without one)"""
    if min_criterion not in _MIN_CRITERIA:
        raise ValueError('{} is not a valid criterion'.format(min_criterion))
    dev = _dev(pred, 'pred')
    _dev(target, 'target')
    if pred.dim() != 4 or pred.shape[-1] != 2 or target.dim() != 3 or tuple(target.shape) != (pred.shape[0],) + tuple(pred.shape[2:]):
        raise InfgenHipError(f'need pred [N, M, T, 2] and target [N, T, 2], got {tuple(pred.shape)}, {tuple(target.shape)}')
    N, M, T = (int(v) for v in pred.shape[:3])
    if valid_mask is None:
        valid_mask = torch.ones(N, T, dtype=torch.bool, device=dev)
    if tuple(valid_mask.shape) != (N, T) or (prob is not None and tuple(prob.shape) != (N, M)):
        raise InfgenHipError(f'need valid_mask [N, T] = {(N, T)} and prob [N, M] = {(N, M)}, got {tuple(valid_mask.shape)}'
                             + ('' if prob is None else f', {tuple(prob.shape)}'))
    p, q = pred.to(torch.float32).contiguous(), target.to(torch.float32).contiguous()
    v = _bytes(valid_mask, 'valid_mask', dev).contiguous()
    w = None
    if prob is not None:
        _dev(prob, 'prob')
        w = prob.to(torch.float32).contiguous()
    owner = ade if ade is not None else fde
    _lib.check(_lib.load().infgen_multi_traj_error(p.data_ptr(), q.data_ptr(), w.data_ptr() if w is not None else None, v.data_ptr(),
                                                   N, M, T, int(owner.max_guesses), int(bool(keep_invalid_final_step)),
                                                   _MIN_CRITERIA[min_criterion],
                                                   ade._state_buf(dev).data_ptr() if ade is not None else None,
                                                   fde._state_buf(dev).data_ptr() if fde is not None else None,
                                                   owner._scratch_buf(dev).data_ptr(), _stream(dev)), 'infgen_multi_traj_error')


class _MultiTrajMetric(_DeviceMetric):
    _slots = 2
    _float_slots = (0,)

    def __init__(self, max_guesses: int = 6, **kwargs) -> None:
        super().__init__(**kwargs)
        self.max_guesses = max_guesses

    sum = property(lambda self: self._state_buf().view(torch.float64)[0])
    count = property(lambda self: self._state_buf()[1])

    def compute(self) -> torch.Tensor:
        b = self._state_buf()
        return b.view(torch.float64)[0] / b[1]


class minMultiFDE(_MultiTrajMetric):
    """reference :339-364: over the rows ``valid_filter`` keeps, the minimum over the ``max_guesses`` most probable modes of the
    distance at the row's last valid step (``topk`` ties: the lower index)"""

    def update(self, pred: torch.Tensor, target: torch.Tensor, prob: Optional[torch.Tensor] = None,
               valid_mask: Optional[torch.Tensor] = None, keep_invalid_final_step: bool = True) -> None:
        update_multi_traj_metrics(None, self, pred, target, prob, valid_mask, keep_invalid_final_step)


class minMultiADE(_MultiTrajMetric):
    """reference :393-427: the masked mean distance of the guess with the smallest final error (``min_criterion='FDE'``, first
    minimum) or the smallest masked mean over the guesses (``'ADE'``); any other criterion raises ValueError like the reference"""

    def update(self, pred: torch.Tensor, target: torch.Tensor, prob: Optional[torch.Tensor] = None,
               valid_mask: Optional[torch.Tensor] = None, keep_invalid_final_step: bool = True,
               min_criterion: str = 'FDE') -> None:
        update_multi_traj_metrics(self, None, pred, target, prob, valid_mask, keep_invalid_final_step, min_criterion)


class AverageMeter(_DeviceMetric):
    """reference :470-482"""
    _slots = 2
    _float_slots = (0,)

    def update(self, val: torch.Tensor) -> None:
        dev = _dev(val, 'val')
        v = val.to(torch.float32).contiguous().reshape(-1)
        _lib.check(_lib.load().infgen_average_meter(v.data_ptr(), v.numel(), self._state_buf(dev).data_ptr(),
                                                    self._scratch_buf(dev).data_ptr(), _stream(dev)), 'infgen_average_meter')

    def compute(self) -> torch.Tensor:
        b = self._state_buf()
        return b.view(torch.float64)[0] / b[1]


class StateAccuracy(_DeviceMetric):
    """reference :485-559.  state: valid, valid_count, invalid, invalid_count"""
    _slots = 4

    def __init__(self, state_token: Dict[str, int], **kwargs) -> None:
        super().__init__(**kwargs)
        self.invalid_state = int(state_token['invalid'])
        self.valid_state = int(state_token['valid'])
        self.enter_state = int(state_token['enter'])
        self.exit_state = int(state_token['exit'])

    def update(self, state_idx: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> None:
        dev = _dev(state_idx, 'state_idx')
        s, s64, ld = _rows(state_idx, 'state_idx', dev)
        N, T = s.shape
        m, ldm = None, 0
        if valid_mask is not None:
            m = _bytes(valid_mask, 'valid_mask', dev)
            if tuple(m.shape) != (N, T):
                raise InfgenHipError(f'valid_mask {tuple(m.shape)} does not match state_idx {(N, T)}')
            if T > 1 and m.stride(1) != 1:
                m = m.contiguous()
            ldm = m.stride(0) if N > 1 else T
            if ldm < T:
                m, ldm = m.contiguous(), T
        _lib.check(_lib.load().infgen_state_accuracy(s.data_ptr(), s64, N, T, ld, m.data_ptr() if m is not None else None, ldm,
                                                     self.invalid_state, self.valid_state, self.enter_state, self.exit_state,
                                                     self._state_buf(dev).data_ptr(), _stream(dev)), 'infgen_state_accuracy')

    @property
    def valid(self):
        return self._state_buf()[0]

    @property
    def valid_count(self):
        return self._state_buf()[1]

    @property
    def invalid(self):
        return self._state_buf()[2]

    @property
    def invalid_count(self):
        return self._state_buf()[3]

    def compute(self) -> Dict[str, torch.Tensor]:
        b = self._state_buf()
        return {'valid': b[0] / b[1],
                'invalid': b[2] / b[3],
                }

    def __repr__(self):
        head = "Results of " + self.__class__.__name__
        results = self.compute()
        body = [
            "valid: {}".format(results['valid'].cpu()),
            "invalid: {}".format(results['invalid'].cpu()),
        ]
        _repr_indent = 4
        lines = [head] + [" " * _repr_indent + line for line in body]
        return "\n".join(lines)


class NumInsertAccuracy(StateAccuracy):
    """reference :618-695: the same computation as StateAccuracy under another name (the same kernel)"""


class GridOverlapRate(_DeviceMetric):
    """reference :562-615.  ``update`` takes an optional ``ptr`` [G + 1] of row ranges: every range is scored as the reference scores
    one call (``num_exceed_seed_t`` once per group); without it everything given is one group, as in the reference.
    ``grid_size``: cells of the tokenizer's grid (indices in [0, grid_size), -1 = out of range); default: the kernel's limit."""

    def __init__(self, num_step, state_token, seed_size, grid_size: Optional[int] = None, **kwargs) -> None:
        super().__init__(**kwargs)
        self.num_step = int(num_step)
        self.enter_state = int(state_token['enter'])
        self.seed_size = seed_size
        self.grid_size = int(grid_size) if grid_size is not None else _lib.GRID_OVERLAP_MAX_CELLS
        self._slots = 4 * self.num_step

    def update(self, state_token: torch.Tensor, grid_index: torch.Tensor, ptr: Optional[torch.Tensor] = None) -> None:
        dev = _dev(state_token, 'state_token')
        s, s64, lds = _rows(state_token, 'state_token', dev)
        g, g64, ldg = _rows(grid_index, 'grid_index', dev)
        if s.shape[0] != g.shape[0] or s.shape[1] < self.num_step or g.shape[1] < self.num_step:
            raise InfgenHipError(f'state_token {tuple(s.shape)} / grid_index {tuple(g.shape)} need equal rows and at least '
                                 f'{self.num_step} columns')
        n_group, p = 1, None
        if ptr is not None:
            p = torch.as_tensor(ptr).to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
            n_group = p.numel() - 1
        _lib.check(_lib.load().infgen_grid_overlap(s.data_ptr(), s64, max(lds, self.num_step), g.data_ptr(), g64,
                                                   max(ldg, self.num_step), s.shape[0], self.num_step,
                                                   p.data_ptr() if p is not None else None, n_group, self.grid_size,
                                                   self.enter_state, int(self.seed_size), self._state_buf(dev).data_ptr(),
                                                   _stream(dev)), 'infgen_grid_overlap')

    def _table(self):
        return self._state_buf().view(4, self.num_step)

    num_overlap_t = property(lambda self: self._table()[0])
    num_insert_agent_t = property(lambda self: self._table()[1])
    num_total_agent_t = property(lambda self: self._table()[2])
    num_exceed_seed_t = property(lambda self: self._table()[3])

    def compute(self) -> Dict[str, torch.Tensor]:
        overlap_rate_t = self.num_overlap_t / self.num_insert_agent_t
        overlap_rate_t.nan_to_num_()
        return {'num_overlap_t': self.num_overlap_t,
                'num_insert_agent_t': self.num_insert_agent_t,
                'num_total_agent_t': self.num_total_agent_t,
                'overlap_rate_t': overlap_rate_t,
                'num_exceed_seed_t': self.num_exceed_seed_t,
                }

    def __repr__(self):
        head = "Results of " + self.__class__.__name__
        results = self.compute()
        body = [
            "num_overlap_t: {}".format(results['num_overlap_t'].tolist()),
            "num_insert_agent_t: {}".format(results['num_insert_agent_t'].tolist()),
            "num_total_agent_t: {}".format(results['num_total_agent_t'].tolist()),
            "overlap_rate_t: {}".format(results['overlap_rate_t'].tolist()),
            "num_exceed_seed_t: {}".format(results['num_exceed_seed_t'].tolist()),
        ]
        _repr_indent = 4
        lines = [head] + [" " * _repr_indent + line for line in body]
        return "\n".join(lines)


def masked_cross_entropy_sums(logits: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, weight: Optional[torch.Tensor] = None,
                              label_smoothing: float = 0.0) -> torch.Tensor:
    """-> float64 [3] on the device: S1 = sum w_y (-log p_y), S2 = sum_i sum_c w_c (-log p_ic) (0 unless label_smoothing), S3 = sum w_y
    over the rows with mask != 0.  logits [..., C] float32 (rows read in place when the inner stride is 1), target / mask [...]"""
    dev = _dev(logits, 'logits')
    _dev(target, 'target')
    C = int(logits.shape[-1]) if logits.dim() else 0
    x = logits if logits.dtype == torch.float32 else logits.to(torch.float32)
    if x.dim() != 2:
        x = x.reshape(-1, max(C, 1))
    if C > 1 and x.stride(1) != 1:
        x = x.contiguous()
    R = x.shape[0]
    ld = x.stride(0) if R > 1 else C
    if ld < C:
        x, ld = x.contiguous(), C
    t, t64, _ = _rows(target.reshape(-1, 1), 'target', dev)
    t = t.contiguous()
    m = _bytes(mask, 'mask', dev).reshape(-1).contiguous()
    if t.shape[0] != R or m.shape[0] != R:
        raise InfgenHipError(f'logits have {R} rows, target {t.shape[0]}, mask {m.shape[0]}')
    w = None
    if weight is not None:
        w = weight.to(device=dev, dtype=torch.float32).contiguous()
        if w.numel() != C:
            raise InfgenHipError(f'weight has {w.numel()} entries for {C} classes')
    acc = torch.zeros(3, dtype=torch.float64, device=dev)
    scratch = torch.empty(_lib.VM_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().infgen_masked_cross_entropy(x.data_ptr(), ld, t.data_ptr(), t64, m.data_ptr(),
                                                       w.data_ptr() if w is not None else None, R, C, float(label_smoothing),
                                                       acc.data_ptr(), scratch.data_ptr(), _stream(dev)),
               'infgen_masked_cross_entropy')
    return acc


def masked_cross_entropy(logits: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, weight: Optional[torch.Tensor] = None,
                         label_smoothing: float = 0.0) -> torch.Tensor:
    """``torch.nn.CrossEntropyLoss(weight, label_smoothing=eps, reduction='mean')(logits[mask], target[mask])`` as a 0-dim float64
    device tensor, without the gather and without a host read: ((1 - eps) S1 + eps / C S2) / S3; NaN when no row is selected"""
    s = masked_cross_entropy_sums(logits, target, mask, weight, label_smoothing)
    eps, C = float(label_smoothing), int(logits.shape[-1])
    return ((1.0 - eps) * s[0] + (eps / C) * s[1]) / s[2]
