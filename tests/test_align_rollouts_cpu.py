"""`align_rollouts` on per-copy dicts whose row counts differ (what `InfGenDecoder.inference_rollouts` returns for a Batch with
insertion: every copy inserts its own agents): plain torch, so checked on the CPU with synthetic dicts whose values encode
(copy, graph, row).  Real rows must land at the new offsets of their graph, the rows a copy lacks must be invalid, in state 0
with id -1, and `format_rollouts` must stack the result."""
import torch

T, T2 = 21, 4
ROW_KEYS = ('pred_valid', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_z', 'eval_shape', 'pred_type', 'next_state_idx',
            'agent_id')


def _copy(j, counts, ego_local, single=False):
    """the dict of copy ``j`` with ``counts[g]`` rows in graph g; every value is code = 10000 * (j + 1) + 100 * g + row (+ small
    per-column offsets), so a moved row is recognised wherever it lands"""
    code = torch.tensor([10000 * (j + 1) + 100 * g + i for g, c in enumerate(counts) for i in range(c)])
    n = code.numel()
    f = code.float()
    d = dict(pred_valid=torch.ones(n, T, dtype=torch.bool), pos_a=f[:, None, None] + torch.arange(T2 * 2).reshape(T2, 2) * 0.01,
             head_a=f[:, None] + torch.arange(T2) * 0.01, pred_traj=f[:, None, None] + torch.arange(T * 2).reshape(T, 2) * 0.001,
             pred_head=f[:, None] + 0.5, pred_z=f[:, None].expand(n, T).clone(), eval_shape=f[:, None] + torch.arange(3) * 0.1,
             pred_type=code % 3, next_state_idx=1 + (code[:, None] + torch.arange(T2)) % 3, agent_id=code.clone(),
             num_inserted=torch.tensor(counts), log_message='copy %d' % j)
    if single:
        d['ego_index'] = ego_local[0]
        return d
    ptr = torch.tensor([0] + list(counts)).cumsum(0)
    d.update(agent_ptr=ptr, agent_batch=torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)),
             ego_index=ptr[:-1] + torch.tensor(ego_local))
    return d


def test_rows_move_to_their_graphs_new_offsets_and_missing_rows_are_padding():
    from infgen_amd.metrics import align_rollouts, format_rollouts
    counts = [[4, 2, 5], [5, 2, 3], [4, 3, 5]]                     # per copy, per graph: graph 0 grows in copy 1, graph 1 in copy 2
    ego = [3, 0, 2]                                                 # local row of the ego in every graph (present in every copy)
    copies = [_copy(j, c, ego) for j, c in enumerate(counts)]
    out, top, per_copy = align_rollouts(copies, return_counts=True)
    assert top == [5, 3, 5] and per_copy == [[4, 5, 4], [2, 2, 3], [5, 3, 5]]
    new_ptr = [0, 5, 8, 13]
    want_batch = torch.tensor([0] * 5 + [1] * 3 + [2] * 5)
    for j, (src, got) in enumerate(zip(copies, out)):
        assert got['agent_ptr'].tolist() == new_ptr and torch.equal(got['agent_batch'], want_batch)
        assert got['log_message'] == src['log_message'] and got['num_inserted'] is src['num_inserted']     # other keys ride along
        old_ptr = src['agent_ptr'].tolist()
        real = torch.zeros(13, dtype=torch.bool)
        for g in range(3):
            c = counts[j][g]
            real[new_ptr[g]:new_ptr[g] + c] = True
            for k in ROW_KEYS:
                assert got[k].shape[0] == 13 and got[k].dtype == src[k].dtype and got[k].shape[1:] == src[k].shape[1:], k
                assert torch.equal(got[k][new_ptr[g]:new_ptr[g] + c], src[k][old_ptr[g]:old_ptr[g + 1]]), (j, g, k)
        # the rows this copy lacks: never valid, state 0 (invalid), id -1, zeros elsewhere
        assert int((~real).sum()) == 13 - sum(counts[j])
        assert not bool(got['pred_valid'][~real].any()) and bool((got['next_state_idx'][~real] == 0).all())
        assert bool((got['agent_id'][~real] == -1).all())
        for k in ('pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_z', 'eval_shape', 'pred_type'):
            assert bool((got[k][~real] == 0).all()), k
        # the ego rows follow their graphs
        assert torch.equal(got['agent_id'][got['ego_index']], src['agent_id'][src['ego_index']])
        assert got['ego_index'].tolist() == [new_ptr[g] + ego[g] for g in range(3)]
    assert align_rollouts(copies)[1]['agent_id'].tolist() == out[1]['agent_id'].tolist()                   # same without the counts
    # ... and format_rollouts stacks them: [rows][copies], av_id per graph from the ego rows
    f = format_rollouts({'scenario_id': ['a', 'b', 'c']}, out)
    assert f['pred_traj'].shape == (13, 3, T, 2) and f['pred_state'].shape == (13, 3, T2) and f['agent_id'].shape == (13, 3)
    assert torch.equal(f['agent_batch'], want_batch)
    assert f['av_id'].tolist() == [10000 + 3, 10000 + 100, 10000 + 202]
    assert f['agent_id'][:, 1].tolist() == out[1]['agent_id'].tolist()
    assert f['pred_valid'].any(2).sum(0).tolist() == [sum(c) for c in counts]


def test_equal_layouts_are_returned_as_they_are():
    from infgen_amd.metrics import align_rollouts
    copies = [_copy(j, [4, 2, 5], [3, 0, 2]) for j in range(3)]
    out = align_rollouts(copies)
    assert all(a is b for a, b in zip(out, copies))
    out, top, per_copy = align_rollouts(copies, return_counts=True)
    assert all(a is b for a, b in zip(out, copies)) and top == [4, 2, 5] and per_copy == [[4] * 3, [2] * 3, [5] * 3]
    # the same total with different graphs' rows is not an equal layout
    moved = [_copy(0, [4, 2, 5], [3, 0, 2]), _copy(1, [5, 2, 4], [3, 0, 2])]
    out, top, per_copy = align_rollouts(moved, return_counts=True)
    assert top == [5, 2, 5] and per_copy == [[4, 5], [2, 2], [5, 4]]
    assert out[0]['agent_id'].tolist() == [10000, 10001, 10002, 10003, -1, 10100, 10101, 10200, 10201, 10202, 10203, 10204]
    assert out[1]['agent_id'].tolist() == [20000, 20001, 20002, 20003, 20004, 20100, 20101, 20200, 20201, 20202, 20203, -1]


def test_single_graph_copies_are_padded_at_their_end():
    """one scene with insertion and several rollouts: no agent_ptr, ego_index a plain int"""
    from infgen_amd.metrics import align_rollouts, format_rollouts
    sizes = [4, 6, 5]
    copies = [_copy(j, [n], [2], single=True) for j, n in enumerate(sizes)]
    out, top, per_copy = align_rollouts(copies, return_counts=True)
    assert top == [6] and per_copy == [sizes]
    for src, got, n in zip(copies, out, sizes):
        assert 'agent_ptr' not in got and 'agent_batch' not in got and got['ego_index'] == 2
        for k in ROW_KEYS:
            assert got[k].shape[0] == 6 and torch.equal(got[k][:n], src[k]), k
        assert not bool(got['pred_valid'][n:].any()) and bool((got['next_state_idx'][n:] == 0).all())
        assert bool((got['agent_id'][n:] == -1).all()) and bool((got['pred_traj'][n:] == 0).all())
    assert out[1] is copies[1]                                     # the largest copy needs nothing
    f = format_rollouts({'scenario_id': ['a']}, out)
    assert f['pred_traj'].shape == (6, 3, T, 2) and f['av_id'] == 10002 and f['agent_batch'].tolist() == [0] * 6
    same = [_copy(j, [5], [2], single=True) for j in range(2)]
    assert all(a is b for a, b in zip(align_rollouts(same), same))
