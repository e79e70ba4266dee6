"""CPU tests for the MAP event path (Viterbi): the torch recursion of
``EventSegment._viterbi_batch`` and the public ``decode`` /
``decode_regions`` built on it.

The rules under test (see ``_viterbi_batch``): a state advances from its
chain predecessor only when that is strictly better than the self loop,
the final state is the lowest k at the maximum, and the score is the
joint log-probability of the returned path.
"""

import itertools

import numpy as np
import pytest
import torch

from brainiak_amd.eventseg.event import (EventSegment, NotFittedError,
                                         _ChainGraph, _viterbi_torch)


def _logprob(B, T, K, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return -torch.randn((B, T, K), generator=g,
                        dtype=torch.float64).abs() * scale


def _model(chains):
    chains = np.asarray(chains)
    return EventSegment(len(chains), event_chains=chains, device="cpu")


def _assert_valid_path(path, graph):
    """Starts at a head, ends at a tail, every step stays or advances."""
    pred = graph.pred.numpy()
    succ = graph.succ.numpy()
    assert pred[path[0]] < 0
    assert succ[path[-1]] < 0
    for a, b in zip(path[:-1], path[1:]):
        assert b == a or b == succ[a]


def _is_valid_path(path, graph):
    try:
        _assert_valid_path(path, graph)
    except AssertionError:
        return False
    return True


# -- brute force ------------------------------------------------------------

def _brute_force(lp, graph):
    """Best of all K^T paths under the dense transition matrix."""
    T, K = lp.shape
    logP = graph.logP.numpy()
    ls = graph.log_start.numpy()
    le = graph.log_end.numpy()
    paths = np.array(list(itertools.product(range(K), repeat=T)))
    with np.errstate(invalid="ignore"):
        sc = ls[paths[:, 0]] + lp[0, paths[:, 0]]
        for t in range(1, T):
            sc = sc + logP[paths[:, t - 1], paths[:, t]]
            sc = sc + lp[t, paths[:, t]]
        sc = sc + le[paths[:, -1]]
    best = int(np.argmax(sc))
    # the winner must be unique for path equality to be a fair demand
    assert np.sum(sc == sc[best]) == 1
    return paths[best], float(sc[best])


@pytest.mark.parametrize("chains", [
    pytest.param([0, 0, 0], id="K3-single-chain"),
    pytest.param([0, 1, 0, 1], id="K4-alternating-chains"),
    pytest.param([0, 1, 1, 0, 1], id="K5-interleaved-two-chains"),
])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_matches_brute_force(chains, seed):
    T = 6
    K = len(chains)
    lp = _logprob(1, T, K, 100 + seed)
    es = _model(chains)
    path, score = es._viterbi_batch(lp)
    graph = es._chain_graph(T, torch.device("cpu"))
    ref_path, ref_score = _brute_force(lp[0].numpy(), graph)
    assert np.array_equal(path[0].numpy(), ref_path)
    assert abs(float(score[0]) - ref_score) <= 1e-12


# -- structural validity ----------------------------------------------------

@pytest.mark.parametrize("chains", [
    pytest.param([0] * 8, id="single-chain"),
    pytest.param([1, 0, 1, 0, 0, 1, 1, 0], id="interleaved-chains"),
])
def test_paths_are_valid_and_bounded_by_ll(chains):
    B, T, K = 32, 40, 8
    lp = _logprob(B, T, K, 7)
    es = _model(chains)
    path, score = es._viterbi_batch(lp)
    _, ll = es._forward_backward_batch(lp)
    graph = es._chain_graph(T, torch.device("cpu"))
    assert path.shape == (B, T) and score.shape == (B,)
    assert score.dtype == torch.float64
    assert not torch.is_floating_point(path)
    for b in range(B):
        _assert_valid_path(path[b].numpy(), graph)
    assert torch.isfinite(score).all()
    assert (score <= ll + 1e-9).all()
    # compat attributes are set as the forward-backward path sets them
    assert es.P.shape == (K + 1, K + 1)
    assert es.p_start.shape == (K + 1,) and es.p_end.shape == (K + 1,)


def test_score_is_the_joint_logprob_of_the_returned_path():
    B, T, K = 4, 25, 5
    lp = _logprob(B, T, K, 11)
    es = _model([0] * K)
    path, score = es._viterbi_batch(lp)
    graph = es._chain_graph(T, torch.device("cpu"))
    logP = graph.logP.numpy()
    for b in range(B):
        z = path[b].numpy()
        x = lp[b].numpy()
        sc = graph.log_start.numpy()[z[0]] + x[0, z[0]]
        for t in range(1, T):
            sc = (sc + logP[z[t - 1], z[t]]) + x[t, z[t]]
        sc = sc + graph.log_end.numpy()[z[-1]]
        assert abs(float(score[b]) - sc) <= 1e-12 * max(1.0, abs(sc))


def test_exact_tie_keeps_the_self_loop():
    """K=2, T=3, lp == 0: the two valid paths 0,0,1 and 0,1,1 score
    ``log_self + log_adv`` and ``log_adv + log_self`` — equal bit for
    bit, since one fp addition commutes.  State 1 at t=2 therefore sees
    va == vs, and the strict comparison keeps its self loop."""
    es = _model([0, 0])
    path, score = es._viterbi_batch(torch.zeros((1, 3, 2),
                                                dtype=torch.float64))
    g = es._chain_graph(3, torch.device("cpu"))
    assert path[0].tolist() == [0, 1, 1]
    assert float(score[0]) == float(g.log_self[0] + g.log_adv[0])


def test_exact_tie_of_final_states_takes_the_lowest():
    """Three one-event chains and lp == 0: all final states tie."""
    es = _model([0, 1, 2])
    path, score = es._viterbi_batch(torch.zeros((2, 4, 3),
                                                dtype=torch.float64))
    assert (path == 0).all()
    assert torch.isfinite(score).all()


def test_flat_observations_give_a_valid_path():
    T, K = 40, 8
    es = _model([0] * K)
    path, score = es._viterbi_batch(torch.zeros((1, T, K),
                                                dtype=torch.float64))
    _assert_valid_path(path[0].numpy(),
                       es._chain_graph(T, torch.device("cpu")))
    assert torch.isfinite(score).all()


def test_pinned_sequence_where_argmax_is_not_a_path():
    """The reason for ``decode``: argmax of the posterior marginals of
    this seeded sequence is no left-to-right path, the MAP path is."""
    T, V, K = 40, 12, 8
    rng = np.random.RandomState(4)        # pinned: see the premise below
    es = EventSegment(K, device="cpu")
    es.set_event_patterns(rng.randn(V, K))
    data = rng.randn(T, V)
    graph = es._chain_graph(T, torch.device("cpu"))

    seg, ll = es.find_events(data, var=1.0)
    labels = seg.argmax(axis=1)
    # the premise: the marginals' argmax steps back (1 -> 0) and skips
    # an event (2 -> 4)
    assert not _is_valid_path(labels, graph)
    assert np.any(np.diff(labels) < 0) and np.any(np.diff(labels) > 1)

    events, logp = es.decode(data, var=1.0)
    assert events.dtype == np.int64 and events.shape == (T,)
    _assert_valid_path(events, graph)
    assert np.isfinite(logp) and logp <= ll + 1e-9


# -- public methods ---------------------------------------------------------

def _block_data(rng, K, L, V, noise):
    patterns = rng.randn(K, V) * 2
    labels = np.repeat(np.arange(K), L)
    return patterns[labels] + noise * rng.randn(K * L, V), labels


def test_decode_recovers_clean_block_structure(seeded_rng):
    K, L, V = 5, 12, 30
    data, labels = _block_data(seeded_rng, K, L, V, 0.1)
    es = EventSegment(K, n_iter=30, device="cpu").fit(data.copy())
    events, logp = es.decode(data)
    assert events.dtype == np.int64
    assert np.array_equal(events, labels)
    _, ll = es.find_events(data)
    assert isinstance(logp, float) and logp <= ll + 1e-9


def test_decode_regions_equals_per_region_decode(seeded_rng):
    rng = seeded_rng
    K, V = 4, 20
    # ragged T: two shape groups, interleaved in input order
    datasets = [_block_data(rng, K, L, V, 0.4)[0]
                for L in (10, 13, 10, 13, 10)]
    proto = EventSegment(K, n_iter=8, device="cpu")
    models = proto.fit_regions(datasets)
    events, logps = proto.decode_regions(models, datasets)
    assert len(events) == len(datasets) and logps.shape == (5,)
    for mdl, d, ev, lpth in zip(models, datasets, events, logps):
        ref_ev, ref_logp = mdl.decode(d)
        assert ev.dtype == np.int64 and ev.shape == (d.shape[0],)
        assert np.array_equal(ev, ref_ev)
        assert abs(lpth - ref_logp) <= 1e-9 * max(1.0, abs(ref_logp))
    # var override reaches the observation model
    ev_v, logp_v = proto.decode_regions(models, datasets, var=2.0)
    ref = models[1].decode(datasets[1], var=2.0)
    assert np.array_equal(ev_v[1], ref[0])
    assert abs(logp_v[1] - ref[1]) <= 1e-9 * max(1.0, abs(ref[1]))
    with pytest.raises(ValueError):
        proto.decode_regions(models[:2], datasets)


def test_decode_with_chains_stays_inside_one_chain(seeded_rng):
    rng = seeded_rng
    T, V = 50, 20
    chains = np.array([0, 0, 1, 1])
    for _ in range(5):
        es = EventSegment(4, event_chains=chains, device="cpu")
        es.set_event_patterns(rng.randn(V, 4))
        events, logp = es.decode(rng.randn(T, V), var=1.0)
        assert len(np.unique(chains[events])) == 1
        _assert_valid_path(events, _ChainGraph(chains, T, "cpu"))
        assert np.isfinite(logp)


def test_too_short_sequence_scores_neg_inf():
    """T < K: no path reaches the tail.  A chain graph built for T
    itself refuses such a T ("Too few timepoints"), so the recursion is
    given one built for a longer sequence."""
    T, K = 5, 8
    graph = _ChainGraph(np.zeros(K), 40, torch.device("cpu"))
    path, score = _viterbi_torch(_logprob(2, T, K, 5), graph)
    assert path.shape == (2, T)
    assert torch.isneginf(score).all()
    assert ((path >= 0) & (path < K)).all()


def test_too_short_sequence_raises_like_find_events(seeded_rng):
    es = EventSegment(8, device="cpu")
    es.set_event_patterns(seeded_rng.randn(10, 8))
    data = seeded_rng.randn(5, 10)
    with pytest.raises(ValueError, match="Too few timepoints"):
        es.find_events(data, var=1.0)
    with pytest.raises(ValueError, match="Too few timepoints"):
        es.decode(data, var=1.0)


def test_decode_not_fitted_errors(seeded_rng):
    data = seeded_rng.randn(20, 10)
    es = EventSegment(3, device="cpu")
    with pytest.raises(NotFittedError):
        es.decode(data)                   # no variance
    with pytest.raises(NotFittedError):
        es.decode(data, var=1.0)          # no patterns
    es.set_event_patterns(seeded_rng.randn(10, 3))
    with pytest.raises(NotFittedError):
        es.decode(data)                   # patterns, still no variance
    events, _ = es.decode(data, var=1.0)
    assert events.shape == (20,)


def test_k65_runs_on_the_torch_path():
    B, T, K = 2, 80, 65
    es = _model([0] * K)
    path, score = es._viterbi_batch(_logprob(B, T, K, 9))
    graph = es._chain_graph(T, torch.device("cpu"))
    for b in range(B):
        _assert_valid_path(path[b].numpy(), graph)
    assert torch.isfinite(score).all()
