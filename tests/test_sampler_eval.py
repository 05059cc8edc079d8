"""The evaluation half of TrainedModelSampler (generation/sampler.py:110-138, 171-368) and the
Metrics class (evaluation/metrics.py:50-214) for the ROCKET feature extractor: features of
the train / test sets, of reconstructions, of stochastic variants and of generated samples,
FID between feature sets and the TSGBench statistics, on a small stage-2 checkpoint
(test_checkpoint's builder, as test_fidelity_enhancer._sampler)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

N_KERNELS = 50


def _data():
    rng = np.random.default_rng(3)
    X_train = np.cumsum(rng.standard_normal((20, 6, 64)), -1).astype(np.float32) * 0.1
    X_test = np.cumsum(rng.standard_normal((12, 6, 64)), -1).astype(np.float32) * 0.1
    return X_train, np.arange(20) % 5, X_test, np.arange(12) % 5


def _regenerated_kernels(build=None):
    """The kernels np.random.seed(0) leads to: `build` first repeats whatever drew from
    np.random before them (the Snake activations' initial values, as in the reference)."""
    from timevqvae.evaluation import generate_kernels
    np.random.seed(0)
    if build is not None:
        build()
    return generate_kernels(64, N_KERNELS)


def _features(x, kernels, dtype):
    """The reference's feature recipe on the host: channel 0, ROCKET, L2-normalised rows."""
    from timevqvae.evaluation import apply_kernels
    z = apply_kernels(np.asarray(x)[:, 0, :].astype(np.float64), kernels)
    return F.normalize(torch.from_numpy(z).to(dtype), p=2, dim=-1).numpy()


@pytest.fixture(scope="module")
def built(tmp_path_factory, cuda):
    """(sampler with the evaluation half, a builder of the same sampler without it)."""
    from test_checkpoint import _build_stage2, _stage2_cfg
    from test_fidelity_enhancer import CFG, _model
    from timevqvae.generation import TrainedModelSampler
    tmp_path = tmp_path_factory.mktemp("sampler_eval")
    cfg = _stage2_cfg()
    cfg["fidelity_enhancer"] = dict(CFG["fidelity_enhancer"])
    s2, p1 = _build_stage2(tmp_path, cfg)
    p2, p3 = tmp_path / "stage2.ckpt", tmp_path / "stage3.ckpt"
    torch.save({"state_dict": s2.state_dict()}, p2)
    fe = _model(6, 64, 4)
    fe.tau.fill_(0.5)  # a tau of the search range, as search_optimal_tau leaves it
    torch.save({"state_dict": {f"fidelity_enhancer.{k}": v for k, v in fe.state_dict().items()}},
               p3)
    X_train, Y_train, X_test, Y_test = _data()

    def build(do_evaluate):
        return TrainedModelSampler(str(p1), str(p2), str(p3), None, input_length=64,
                                   in_channels=6, n_classes=5, batch_size=16, X_train=X_train,
                                   Y_train=Y_train, X_test=X_test, Y_test=Y_test, device=cuda,
                                   config=cfg, feature_extractor_type="rocket",
                                   rocket_num_kernels=N_KERNELS, do_evaluate=do_evaluate)
    np.random.seed(0)
    return build(True), lambda: build(False)


@pytest.fixture(scope="module")
def sampler(built):
    return built[0]


def test_supervised_fcn_evaluation_is_refused_before_any_path_is_read():
    from timevqvae.evaluation import Metrics
    from timevqvae.generation import TrainedModelSampler
    with pytest.raises(NotImplementedError, match="FCN"):
        TrainedModelSampler("/no/such/stage1", "/no/such/stage2", "/no/such/stage3", "/no/such/fcn",
                            64, 6, 5, 16, feature_extractor_type="supervised_fcn", do_evaluate=True)
    with pytest.raises(NotImplementedError, match="FCN"):
        Metrics("/no/such/fcn", 64, 6, 5, 16, None, None, "cpu", "supervised_fcn")


@pytest.mark.gpu
def test_sampler_builds_the_evaluation_state(sampler, built):
    X_train, _, X_test, _ = _data()
    kernels = _regenerated_kernels(built[1])
    assert float(sampler.fidelity_enhancer.tau) == 0.5
    for got, want in zip(sampler.rocket_kernels, kernels):
        np.testing.assert_array_equal(got, want)
    assert sampler.ts_len == 64 and sampler.n_classes == 5
    assert sampler.z_train.shape == (20, 100) and sampler.z_test.shape == (12, 100)
    assert sampler.z_train.dtype == np.float64
    np.testing.assert_allclose(np.linalg.norm(sampler.z_train, axis=1), 1.0, rtol=1e-12)
    # float64 throughout: only the norm's summation order may differ from the host's
    np.testing.assert_allclose(sampler.z_train, _features(X_train, kernels, torch.float64),
                               rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(sampler.z_test, _features(X_test, kernels, torch.float64),
                               rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(sampler.compute_z("test"), sampler.z_test)


@pytest.mark.gpu
def test_sampler_feature_loops(sampler, cuda):
    _, _, X_test, _ = _data()
    with torch.no_grad():
        x_rec = sampler.stage1.forward(batch=(torch.from_numpy(X_test).to(cuda), None),
                                       batch_idx=-1, return_x_rec=True)
    want = _features(x_rec.cpu().numpy(), sampler.rocket_kernels, torch.float64)
    np.testing.assert_allclose(sampler.compute_z_rec("test"), want, rtol=1e-12, atol=1e-15)
    # generated samples arrive as a CPU tensor (sampler.sample's X_new_R)
    np.testing.assert_array_equal(sampler.compute_z_gen(torch.from_numpy(X_test)), sampler.z_test)
    z_svq, x_svq = sampler.compute_z_svq("test")
    assert z_svq.shape == (12, 100) and x_svq.shape == (12, 6, 64)
    assert np.isfinite(z_svq).all() and np.isfinite(x_svq).all()


@pytest.mark.gpu
def test_sampler_scores(sampler):
    from timevqvae.evaluation import (auto_correlation_difference, calculate_fid,
                                      kurtosis_difference, marginal_distribution_difference,
                                      skewness_difference)
    from timevqvae.utils import remove_outliers
    X_train, _, X_test, _ = _data()
    fid = sampler.fid_score(sampler.z_train, sampler.z_test)
    np.testing.assert_array_equal(
        fid, calculate_fid(remove_outliers(sampler.z_train), remove_outliers(sampler.z_test)))
    got = sampler.stat_metrics(X_test, X_train)
    want = (marginal_distribution_difference(X_test, X_train),
            auto_correlation_difference(X_test, X_train), skewness_difference(X_test, X_train),
            kurtosis_difference(X_test, X_train))
    assert tuple(got) == want and all(np.isfinite(got))
    with pytest.raises(NotImplementedError, match="FCN"):
        sampler.inception_score(torch.from_numpy(X_test))


@pytest.mark.gpu
def test_metrics_class(cuda):
    from timevqvae.evaluation import (Metrics, auto_correlation_difference, calculate_fid,
                                      kurtosis_difference, marginal_distribution_difference,
                                      skewness_difference)
    from timevqvae.utils import remove_outliers
    X_train, _, X_test, _ = _data()
    np.random.seed(0)
    m = Metrics(None, 64, 6, 5, 16, X_train, X_test, cuda, "rocket", rocket_num_kernels=N_KERNELS)
    kernels = _regenerated_kernels()
    for got, want in zip(m.rocket_kernels, kernels):
        np.testing.assert_array_equal(got, want)
    assert m.z_train.shape == (20, 100) and m.z_train.dtype == np.float32
    assert m.z_test.shape == (12, 100)
    # float32 normalisation: a few float32 roundings between the device's norm and the host's
    np.testing.assert_allclose(m.z_train, _features(X_train, kernels, torch.float32), rtol=1e-6,
                               atol=1e-9)
    np.testing.assert_allclose(np.linalg.norm(m.z_test.astype(np.float64), axis=1), 1.0, rtol=1e-6)
    np.testing.assert_array_equal(m.compute_z(X_test), m.z_test)
    np.testing.assert_array_equal(m.z_gen_fn(X_test), m.z_test)
    mu, sd = m.compute_z_stat(X_train)
    assert mu.shape == (1, 100) and sd.shape == (1, 100)
    np.testing.assert_array_equal(
        m.fid_score(m.z_train, m.z_test),
        calculate_fid(remove_outliers(m.z_train), remove_outliers(m.z_test)))
    assert tuple(m.stat_metrics(X_test, X_train)) == (
        marginal_distribution_difference(X_test, X_train),
        auto_correlation_difference(X_test, X_train), skewness_difference(X_test, X_train),
        kurtosis_difference(X_test, X_train))
    with pytest.raises(NotImplementedError, match="FCN"):
        m.inception_score(X_test)
