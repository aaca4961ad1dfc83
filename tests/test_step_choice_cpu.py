"""Which BPR step kernel steps batch size B (single/_engine.py layout_for / step_kind / stepped_down), as a table; and the two
properties of the engine's bookkeeping that nothing used to check: the "same call as last time?" comparison sees every switch,
and every attribute the choice reads exists from construction on.  No library, no GPU."""
import dataclasses

import numpy as np
import pytest
import torch

from single import _engine
from single._config import Tuning


def _choose(B, k=128, owners=256, min_owners=0, fits=True, own_failed=False, flow_disabled=False, **switches):
    cfg = dataclasses.replace(Tuning.from_env({}), **switches)
    layout = _engine.layout_for(B, k, cfg, fits, flow_disabled)
    return _engine.step_kind(layout, B, cfg, owners, min_owners, own_failed)


@pytest.mark.parametrize('inputs, kind', [
    (dict(B=64), 'own'),
    (dict(B=256), 'own'),
    (dict(B=257), 'flow'),
    (dict(B=512), 'flow'),
    (dict(B=513), 'bulk'),
    (dict(k=256, B=256), 'own'),
    (dict(k=257, B=64), 'bulk'),
    (dict(own='0', B=256), 'flow'),
    (dict(own='2', B=256), 'own'),
    (dict(flow=False, B=64), 'bulk'),
    (dict(fits=False, B=64), 'bulk'),
    (dict(owners=0, B=256), 'flow'),
    (dict(owners=100, min_owners=128, B=256), 'flow'),
    (dict(owners=128, min_owners=128, B=256), 'own'),
    (dict(own_max_batch=1024, flow_max_batch=512, B=600), 'bulk'),
    (dict(own_max_batch=1024, flow_max_batch=1024, B=1024), 'own'),
    (dict(own_failed=True, B=256), 'flow'),
    (dict(flow_disabled=True, B=64), 'bulk'),
], ids=lambda x: x if isinstance(x, str) else ','.join('%s=%s' % kv for kv in x.items()))
def test_the_kernel_that_steps_a_batch_size(inputs, kind):
    assert _choose(**inputs) == kind


def test_a_forced_layout_counts_for_the_step():
    cfg = Tuning.from_env({})
    assert _engine.step_kind('flow', 2048, cfg, 256, 0, False) == 'flow'       # prepare(B, layout='flow') above flow_max_batch
    assert _engine.step_kind('bulk', 64, cfg, 256, 0, False) == 'bulk'


def test_step_down_sequence_at_batch_256():
    flags = (False, False)                                                      # (K2o failed, flow layout disabled)
    assert _choose(256, own_failed=flags[0], flow_disabled=flags[1]) == 'own'
    for last, then in (('own', 'flow'), ('flow', 'bulk'), ('bulk', 'bulk'), (None, 'bulk')):
        flags = _engine.stepped_down(last, *flags)
        assert _choose(256, own_failed=flags[0], flow_disabled=flags[1]) == then, last
    assert flags == (True, True)
    assert _engine.stepped_down(None, False, False) == (False, True)            # an engine that has not stepped yet: the flow layout goes


def test_the_same_call_comparison_sees_every_switch_and_input():
    inputs = (256, 1, 7, 1, 0, False, False)         # BprEngine._inputs: B, layout_epoch, seed, ranks_on_device, own_min_owners, the two flags
    cfg = Tuning()
    built = _engine._Built(cfg, inputs, step=None)
    assert built.cfg is not vars(cfg) and built.same(cfg, inputs) and built.same(Tuning(), tuple(inputs))
    for f in dataclasses.fields(Tuning):
        old = getattr(cfg, f.name)
        new = (not old) if isinstance(old, bool) else old + 1 if isinstance(old, int) else {'1': '0'}.get(old, old + 'x')
        setattr(cfg, f.name, new)                    # in place, as `e.cfg.own_waves = 7` in the middle of a run
        assert not built.same(cfg, inputs), f.name
        setattr(cfg, f.name, old)
        assert built.same(cfg, inputs), f.name
    for q in range(len(inputs)):
        other = inputs[:q] + ((not inputs[q]) if isinstance(inputs[q], bool) else inputs[q] + 1,) + inputs[q + 1:]
        assert not built.same(cfg, other), q


CHOICE_STATE = ('_own_failed', '_flow_disabled', '_flow_fits', '_owners_by_share', '_last_step_kind', '_step_key', '_step', '_warned_wide',
                '_shadow_icnt', 'tables_invalid', 'ranks_on_device', 'own_min_owners', 'private_side_stream', 'plan_in_order')
SET_FROM_OUTSIDE = ('ranks_on_device', 'own_min_owners', 'private_side_stream', 'plan_in_order', 'step_events', 'tables_invalid',
                    '_last_step_kind', '_flow_ran', 'cfg')


def test_every_attribute_of_the_choice_is_declared_at_construction():
    cpu = torch.device('cpu')
    hp = dict(lu=0.0, li=0.0, lj=0.0, lb=0.0, le=0.0, lr=0.01, mode='l2')
    bpr = _engine.BprEngine(5, 4, 8, hp, device=cpu, seed=1)
    vbpr = _engine.VbprEngine(5, 4, 8, 3, np.ones((4, 3), np.float32), hp, device=cpu, seed=1)
    for name in CHOICE_STATE + SET_FROM_OUTSIDE:
        assert name in vars(bpr), name
    for name in SET_FROM_OUTSIDE + ('_step_key', '_step', '_warned_wide', '_shadow_icnt'):
        assert name in vars(vbpr), name
    # what the callers of either engine read without asking whether it is there (BPR.train, dist.ItemSync)
    assert (vbpr.layout, vbpr.ctl) == (bpr.layout, bpr.ctl) == ('bulk', None)
    assert (bpr.ranks_on_device, bpr.own_min_owners, bpr.private_side_stream, bpr.plan_in_order, bpr.tables_invalid) == (1, 0, False, False, False)
    assert bpr._last_step_kind is None and bpr._flow_ran is False and bpr.step_events is None
    import inspect
    assert 'self._callers = {}' in inspect.getsource(_engine.PlanBuffers.__init__)
    for cls in (_engine.BprEngine, _engine.VbprEngine, _engine.PlanMixin, _engine.PlanBuffers, _engine.PlanPipeline):
        assert '__dict__' not in inspect.getsource(cls), cls.__name__
