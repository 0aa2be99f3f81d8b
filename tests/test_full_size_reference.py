"""CPU checks of tests/full_size_reference.py, the host side of the full-size parity audit: the chunked, threaded oracle labels
equal one oracle call, the row generators are deterministic per seed, and the MIBI-like rows really repeat."""
import numpy as np
import pytest
import torch

from tests import full_size_reference as fr


@pytest.mark.parametrize("n,chunk,threads", [(100_000, 1 << 20, None), (123_457, 30_001, 4), (200_003, 65_536, 3),
                                             (7, 3, 16), (0, 1000, 2)])
def test_oracle_labels_equals_one_oracle_call(oracle, n, chunk, threads):
    x = fr.fov_rows(1, n, 22, 1000, "cpu") if n else torch.empty((0, 22))
    w = fr.data_row_codebook(fr.fov_rows(1, 5_000, 22, 9, "cpu"), 100)
    w[99] = w[3]                                           # a duplicate node: the first one wins, in every chunk
    lab, d, s, cnt = fr.oracle_labels(w, x, chunk_rows=chunk, threads=threads, with_sums=True)
    want_l, want_d = oracle.map_data_to_nodes(w.numpy(), x.double().numpy())
    np.testing.assert_array_equal(lab, want_l)
    np.testing.assert_array_equal(d.view(np.int64), want_d.view(np.int64))
    want_s, want_c = oracle.cluster_sums(x.double().numpy(), want_l, 100)
    np.testing.assert_array_equal(cnt, want_c)
    np.testing.assert_allclose(s, want_s, rtol=1e-12, atol=0)
    lab2, d2 = fr.oracle_labels(w.numpy(), x.to(torch.float16).float(), chunk_rows=chunk, threads=threads)
    np.testing.assert_array_equal(lab2, oracle.map_data_to_nodes(w.numpy(), x.to(torch.float16).double().numpy())[0])


def test_oracle_threads_follow_omp_num_threads(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert fr.oracle_threads() == 3
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert fr.oracle_threads() == 16


@pytest.mark.parametrize("make", [lambda s: fr.fov_rows(2, 20_000, 22, s, "cpu"),
                                  lambda s: fr.fov_rows(1, 30_000, 40, s, "cpu", dtype=torch.float16),
                                  lambda s: fr.cell_rows(50_000, 100, s, "cpu"),
                                  lambda s: fr.mibi_rows(100_000, 22, s, "cpu")])
def test_row_generators_are_deterministic_per_seed(make):
    a, b, other = make(11), make(11), make(12)
    assert torch.equal(a, b)
    assert not torch.equal(a, other)
    assert bool(torch.isfinite(a.float()).all()) and float(a.min()) >= 0.0


def test_mibi_rows_repeat_and_are_sparse():
    x = fr.mibi_rows(200_000, 22, 77, "cpu")
    assert x.dtype == torch.float32 and x.shape == (200_000, 22)
    nnz = (x > 0).sum(dim=1)
    assert int(nnz.min()) == 1 and int(nnz.max()) == 3
    distinct = torch.unique(x, dim=0).shape[0]
    assert distinct < x.shape[0] // 2, f"{distinct} distinct rows of {x.shape[0]}"


def test_cell_rows_restate_the_poisson_table():
    x = fr.cell_rows(200_000, 100, 2000, "cpu")
    zeros = float((x == 0).float().mean())
    assert abs(zeros - np.exp(-3.0)) < 2e-3                     # Poisson(3) counts: P(0) = e^-3
    q = torch.quantile(x[:, :5], 0.999, dim=0)
    assert bool(((q > 0.99) & (q < 1.01)).all())                 # every column divided by its own 99.9 % value


def test_codebook_builders(oracle):
    x = fr.fov_rows(1, 20_000, 22, 5, "cpu")
    w = fr.data_row_codebook(x, 100)
    assert w.dtype == torch.float64 and w.shape == (100, 22)
    _, d = oracle.map_data_to_nodes(w.numpy(), w.numpy())
    assert np.all(d == 0.0)                                      # every node is a row: distance-0 matches
    near = fr.near_pair_codebook(w)
    assert torch.equal(near[:50], w[:50])
    rel = ((near[50:] - w[:50]).abs() / w[:50].abs().clamp(min=1e-300))[w[:50] != 0]
    assert 0.0 < float(rel.median()) < 0.05
    assert torch.equal(fr.first_codebook(x, 100), fr.first_codebook(x, 100))


def test_exact_cluster_sums():
    x = fr.cell_rows(30_000, 100, 3, "cpu")
    labels = torch.from_numpy(np.random.RandomState(0).randint(1, 11, size=30_000).astype(np.int32))
    got = fr.exact_cluster_sums(x, labels, 10)
    want = torch.zeros((10, 100), dtype=torch.float64).index_add_(0, labels.long() - 1, x.double())
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-13)
    # exact: any order gives the same bits
    perm = torch.randperm(30_000)
    assert torch.equal(fr.exact_cluster_sums(x[perm], labels[perm], 10), got)
