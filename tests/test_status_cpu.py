"""What the bindings of K12 to K25 share (tkr_hip.py), without a GPU: the one reader of the status word over every family and every
kind, the one operand check in both exception styles, the one tail of the wrappers with a check= argument."""
import pytest
import torch

ROWS = (0, 1, 2 ** 40)


def _families():
    """(family, messages, raises, the class each defined kind must raise, the word's attributes are a promise of the class)"""
    import tkr_hip as T
    return [('K15', T._GROUP_REFUSED, ValueError, {0: ValueError, 1: ValueError, 2: ValueError, 3: ValueError}),
            ('K17', T._DIV_REFUSED, T.TkrError, {1: T.TkrError}),
            ('K18', T._LINE_REFUSED, T.TkrError, {0: T.TkrError, 1: T.TkrError, 2: T.TkrError, 3: T.TkrError}),
            ('K19', T._ANCHOR_REFUSED, T._ANCHOR_RAISES, {0: T.TkrError, 1: T.TkrError, 3: ValueError}),
            ('K20', T._ALS_REFUSED, T.AlsRefused, {1: T.AlsRefused, 2: T.AlsRefused, 3: T.AlsRefused}),
            ('K24', T._ALS_CG_REFUSED, T.AlsCgRefused, {1: T.AlsCgRefused, 2: T.AlsCgRefused, 3: T.AlsCgRefused}),
            ('K25', T._LMF_REFUSED, T.LmfRefused, {1: T.LmfRefused, 3: T.LmfRefused}),
            ('K22', T._MLP_REFUSED, T.MlpRefused, {1: T.MlpRefused})]


@pytest.mark.parametrize('family', range(8))
def test_every_kind_of_every_family_raises_its_class_and_names_the_row(family):
    import tkr_hip as T
    name, messages, raises, defined = _families()[family]
    what = 'entry_of_' + name
    T.status_check(what, messages, raises, -1)                       # clean: nothing is raised
    for kind in range(4):
        for row in ROWS:
            word = 4 * row + kind
            if kind in defined:
                with pytest.raises(defined[kind]) as info:
                    T.status_check(what, messages, raises, word)
                e = info.value
                assert type(e) is defined[kind]
                assert (e.word, e.row, e.kind) == (word, row, kind)
                assert what in str(e) and str(row) in str(e)
                if name == 'K22':
                    assert e.position == row
                if name in ('K20', 'K24', 'K25'):
                    assert '(kind %d)' % kind in str(e) and isinstance(e, T.AlsRefused) and isinstance(e, T.TkrError)
            else:                                                     # a kind the family does not write: the raw word, by name
                with pytest.raises(T.TkrError) as info:
                    T.status_check(what, messages, raises, word)
                assert type(info.value) is T.TkrError
                assert what in str(info.value) and 'status word %d' % word in str(info.value)


def test_the_tables_keep_their_gaps_and_the_classes_their_bases():
    import tkr_hip as T
    defined = {name: sorted(d) for name, _, _, d in _families()}
    assert defined == dict(K15=[0, 1, 2, 3], K17=[1], K18=[0, 1, 2, 3], K19=[0, 1, 3], K20=[1, 2, 3], K24=[1, 2, 3], K25=[1, 3], K22=[1])
    for name, messages, _, d in _families():
        assert [k for k in range(4) if k < len(messages) and messages[k] is not None] == sorted(d), name
    assert T.AlsRefused.__bases__ == (T.TkrError,) and T.MlpRefused.__bases__ == (T.TkrError,)
    assert T.AlsCgRefused.__bases__ == (T.AlsRefused,) and T.LmfRefused.__bases__ == (T.AlsRefused,)
    assert T.DeviceGroupTooLarge.__bases__ == (T.TkrError,)
    assert T._ALS_CG_REFUSED[1] is T._ALS_REFUSED[1] and T._ALS_CG_REFUSED[2] != T._ALS_REFUSED[2]
    assert T.LINE_MAX_COLS == T.GROUP_MAX_COLS and T.ANCHOR_MAX_T == T.MMR_MAX_POOL
    with pytest.raises(T.TkrError, match='row 12345 of the features'):
        T.fusion_svm_check(12345)
    T.fusion_svm_check(-1)


def test_the_tail_hands_the_word_on_unread_or_reads_it():
    import tkr_hip as T
    result = object()
    clean, refused = torch.tensor([-1]), torch.tensor([4 * 7 + 1])
    assert T._done('x', result, refused, False, T._ALS_REFUSED, T.AlsRefused) == (result, refused)
    assert T._done('x', result, clean, True, T._ALS_REFUSED, T.AlsRefused) is result
    with pytest.raises(T.MlpRefused, match='x: entry 7 of the row list') as info:
        T._done('x', result, refused, True, T._MLP_REFUSED, T.MlpRefused)
    assert info.value.position == 7


# (what is wrong, the operand it is wrong with, (K15 style class, the class of the other families))
BAD = [('not a tensor', [0, 1, 2], (TypeError, 'TkrError'), 'must be a tensor'),
       ('wrong dtype', 'dtype', (TypeError, 'TkrError'), 'must be torch.'),
       ('non-contiguous', 'strided', (ValueError, 'TkrError'), 'must be contiguous'),
       ('wrong rank', 'rank', (ValueError, 'TkrError'), 'dimensions'),
       ('wrong count', 'count', (ValueError, 'TkrError'), 'must hold'),
       ('host tensor', 'host', (ValueError, 'TkrError'), 'must live on the GPU')]


@pytest.mark.parametrize('case', range(len(BAD)))
def test_group_segments_refuses_a_bad_operand_by_name(case):
    """K15 style: TypeError for what is no tensor of the dtype, ValueError for the rest; seg_ptr is the operand"""
    import tkr_hip as T
    _, how, (cls, _), fragment = BAD[case]
    item, like = torch.tensor([1, 2, 3], dtype=torch.int32), torch.tensor([1, 0, 1], dtype=torch.int32)
    seg_ptr = {'dtype': torch.tensor([0, 2, 3], dtype=torch.int32), 'strided': torch.zeros(6, dtype=torch.int64)[::2],
               'rank': torch.zeros((1, 3), dtype=torch.int64), 'count': torch.zeros(0, dtype=torch.int64),
               'host': torch.tensor([0, 2, 3])}.get(how if isinstance(how, str) else '', how)
    with pytest.raises(cls) as info:
        T.group_segments([(seg_ptr, item, like, None)], 2, 10)
    assert type(info.value) is cls and 'group_segments: seg_ptr' in str(info.value) and fragment in str(info.value)


@pytest.mark.parametrize('case', range(len(BAD)))
def test_fusion_svm_sums_refuses_a_bad_operand_by_name(case):
    """the style of the other families: TkrError throughout; D is the operand (W for the count, which D does not have)"""
    import tkr_hip as T
    _, how, _, fragment = BAD[case]
    D = {'dtype': torch.zeros((20, 3), dtype=torch.float64), 'strided': torch.zeros((3, 20)).t(), 'rank': torch.zeros(20),
         'host': torch.zeros((20, 3))}.get(how if isinstance(how, str) else '', how)
    if how == 'count':
        with pytest.raises(T.TkrError) as info:
            T._operand('fusion_svm_sums', 'W', torch.zeros(3, dtype=torch.float64), torch.float64, numel=4, on=T._LATER)
        assert 'fusion_svm_sums: W must hold 4 values' in str(info.value)
        with pytest.raises(T.TkrError, match='partial must hold at least 16 values'):
            T._operand('fusion_svm_sums', 'partial', torch.zeros(15, dtype=torch.float64), torch.float64, at_least=16, on=T._LATER)
        return
    with pytest.raises(T.TkrError) as info:
        T.fusion_svm_sums(D, torch.zeros(4, dtype=torch.float64))
    assert type(info.value) is T.TkrError and 'fusion_svm_sums: D' in str(info.value) and fragment in str(info.value)


def test_the_operand_check_keeps_its_order_and_lets_none_through_only_when_asked():
    import tkr_hip as T
    bad = torch.zeros((3, 20), dtype=torch.float64).t()               # wrong dtype, not contiguous, wrong rank, wrong count, on the host
    for fix, fragment in ((lambda t: t, 'must be torch.float32'), (lambda t: t.float(), 'must be contiguous'),
                          (lambda t: t.float().contiguous(), 'must have 1 dimensions'),
                          (lambda t: t.float().contiguous().reshape(-1), 'must hold 4 values'),
                          (lambda t: t.float().contiguous().reshape(-1)[:4].clone(), 'must live on the GPU')):
        with pytest.raises(T.TkrError, match='e: t ' + fragment):
            T._operand('e', 't', fix(bad), torch.float32, 1, numel=4)
    T._operand('e', 't', None, torch.float32, optional=True)
    with pytest.raises(TypeError, match='e: t must be a tensor'):
        T._operand('e', 't', None, torch.float32, raises=T._STD)
    with pytest.raises(T.TkrError, match='one GPU'):
        T._on_gpu('e', 't', torch.zeros(1))
