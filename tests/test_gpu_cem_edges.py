"""Two edges of SdcEngine.plan_cem beside tests/test_gpu_cem.py: an engine pinned to a stream of its own (use_stream) while probs and
best_seq are filled on torch's current stream, and NaN scores, for which include/sustaindc_hip.h states the outcome: every candidate
has rank 0 and is elite, the divisor stays E, and the incumbent-to-be is the lowest-numbered candidate.  N, M, E, K and the engines
are that file's."""
import pytest

from tests.plan_util import OBJ, _twins
from tests.test_gpu_cem import E, K, M, N, _probs, _same, _seq

pytestmark = pytest.mark.gpu


def test_a_pinned_stream_waits_for_the_tensors_filled_on_the_current_one():
    import torch
    (a, b), _ = _twins(N)
    side = torch.cuda.Stream(device=b.device)
    b.use_stream(side)
    kw = dict(seed=9, draw=2, alpha=0.3, p_min=0.02, **OBJ)
    # the defaults (uniform, do nothing), then a caller's tensors written just before the call
    for given in (False, True):
        ra = a.plan_cem(K, 2, M, E, **(dict(probs=_probs(K, N) * 1.0, best_seq=_seq(K, N) + 0) if given else {}), **kw)
        rb = b.plan_cem(K, 2, M, E, **(dict(probs=_probs(K, N) * 1.0, best_seq=_seq(K, N) + 0) if given else {}), **kw)
        side.synchronize()
        torch.cuda.synchronize()
        _same(ra, rb, "pinned against unpinned, tensors given: %s" % given)
    b.use_stream(None)
    a.close()
    b.close()


def test_nan_scores_make_every_candidate_elite_and_keep_the_incumbent():
    import torch
    (b,), _ = _twins(N, n=1)
    p0, s0 = _probs(K, N), _seq(K, N)
    kw = dict(probs=None, best_seq=None, seed=5, reward_weights=(0.0, 0.0, 0.0), info_weights={"dc_water_usage": float("nan")})
    runs = []
    for _ in range(2):
        kw.update(probs=p0.clone(), best_seq=s0.clone())
        runs.append(b.plan_cem(K, 1, M, E, **kw))
    res = runs[0]
    assert bool(res.cand_score.isnan().all()) and bool(res.best_score.isnan().all())
    assert torch.equal(res.best_seq, s0) and torch.equal(res.action, s0[0])
    # all M candidates are counted, the divisor is E (alpha = 0, p_min = 0)
    q = (res.cand[..., None] == torch.arange(3, device=b.device, dtype=torch.int32)).sum(0).double() / float(E)
    assert torch.equal(res.probs, q / ((q[..., 0] + q[..., 1]) + q[..., 2])[..., None])
    for nm in ("action", "best_seq", "probs", "cand"):
        assert torch.equal(getattr(runs[0], nm), getattr(runs[1], nm)), nm
    b.close()
