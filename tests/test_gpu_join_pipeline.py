"""The opt-in mirrors built on the table join, on the GIAB mini trio: the fused extract-and-subtract stage
(``_extract_child_non_ref_kmers``) against the two stages it replaces, and the parent filter under ``KDF_DEVICE_JOIN=1``
against the default path -- the same counts (51 125 -> 6 679 -> 1 513 -> 630 at k = 31) and the same bytes in every
contract file."""
import os
import shutil

import pytest

from conftest import GIAB

pytestmark = pytest.mark.gpu

CHILD = os.path.join(GIAB, "HG002_child.bam")
MOTHER = os.path.join(GIAB, "HG004_mother.bam")
FATHER = os.path.join(GIAB, "HG003_father.bam")
MIN_CHILD = 3


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _records(fasta_bytes):
    return fasta_bytes.count(b">")


@pytest.fixture(scope="module")
def ref_jf(tmp_path_factory):
    """k -> reference index of mini_ref.fa: the committed Jellyfish file at k = 31, one built on the way of
    tests/test_gpu_long_k_pipeline.py at k = 75"""
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _ensure_ref_jf
    made = {31: os.path.join(GIAB, "mini_ref.fa.k31.jf")}

    def get(k):
        if k not in made:
            tmp = str(tmp_path_factory.mktemp(f"ref{k}"))
            fa = os.path.join(tmp, "mini_ref.fa")
            shutil.copy(os.path.join(GIAB, "mini_ref.fa"), fa)       # nothing is written under tests/golden
            made[k] = _ensure_ref_jf(fa, k, 4)
            assert made[k].startswith(tmp)
        return made[k]
    return get


@pytest.fixture(scope="module")
def two_stage(tmp_path_factory, ref_jf):
    """k -> (n_candidates, n_non_ref, bytes of child_non_ref_kmers.fa) of the two existing stages, under the settings of
    the environment as it is when asked (keyed by them: the default chain runs once)"""
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_kmers_discovery, _subtract_reference_kmers
    done = {}

    def get(k):
        assert not os.environ.get("KDF_DEVICE_JOIN")
        key = (k,) + tuple(os.environ.get(v) for v in ("KDF_KEY_PARTS", "KDF_PREFILTER"))
        if key not in done:
            tmp = str(tmp_path_factory.mktemp(f"two{k}"))
            fa, n = _extract_child_kmers_discovery(CHILD, None, k, MIN_CHILD, 4, tmp)
            out, n2 = _subtract_reference_kmers(ref_jf(k), fa, tmp)
            done[key] = (n, n2, _read(out))
        return done[key]
    return get


def _kmers(fasta_bytes):
    return sorted(fasta_bytes.split(b"\n")[1::2])


def _parents(non_ref_fa, k, tmp, monkeypatch):
    """_filter_parents_discovery -> (n_proband, bytes of after_mother.fa, bytes of proband_unique.fa)"""
    from kmer_denovo_filter_amd.discovery import pipeline
    kept = {}
    remove = pipeline.remove_with_sidecar

    def keeping(path):
        kept[os.path.basename(path)] = _read(path)
        remove(path)
    monkeypatch.setattr(pipeline, "remove_with_sidecar", keeping)
    n, fa = pipeline._filter_parents_discovery(MOTHER, FATHER, None, non_ref_fa, k, 4, tmp, 0)
    monkeypatch.setattr(pipeline, "remove_with_sidecar", remove)
    return n, kept["after_mother.fa"], _read(fa)


def test_fused_stage_k31(tmp_path, two_stage, ref_jf, monkeypatch):
    from kmer_denovo_filter_amd import devkeys
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_non_ref_kmers
    want = two_stage(31)
    assert want[:2] == (51125, 6679)
    tmp = str(tmp_path)
    fa, n_cand, n_non_ref = _extract_child_non_ref_kmers(CHILD, None, ref_jf(31), 31, MIN_CHILD, 4, tmp)
    assert (n_cand, n_non_ref) == (51125, 6679)
    assert fa == os.path.join(tmp, "child_non_ref_kmers.fa") and _read(fa) == want[2]
    assert not os.path.exists(os.path.join(tmp, "child_candidates.fa"))
    dev = devkeys.lookup(fa, 31)                                      # registered for Module 2, as the subtraction does
    assert dev is not None and dev[0].shape[0] == 6679 and dev[1] is None
    n, after_mother, proband = _parents(fa, 31, tmp, monkeypatch)
    assert _records(after_mother) == 1513 and n == _records(proband) == 630


@pytest.mark.parametrize("env", ("KDF_KEY_PARTS=3", "KDF_PREFILTER=1"))
def test_fused_stage_sliced_and_two_pass(env, tmp_path, two_stage, ref_jf, monkeypatch):
    from kmer_denovo_filter_amd.discovery import pipeline
    default = two_stage(31)
    name, value = env.split("=")
    monkeypatch.setenv(name, value)
    want = two_stage(31)                        # the two stages under the same setting (key slices: slice by slice, ascending in each)
    assert want[:2] == (51125, 6679) and _kmers(want[2]) == _kmers(default[2])
    fa, n_cand, n_non_ref = pipeline._extract_child_non_ref_kmers(CHILD, None, ref_jf(31), 31, MIN_CHILD, 4, str(tmp_path))
    assert (n_cand, n_non_ref) == (51125, 6679) and _read(fa) == want[2]
    assert not os.path.exists(os.path.join(str(tmp_path), "child_candidates.fa"))
    assert pipeline.LAST_CHILD_COUNT["mode"] == ("two_pass" if name == "KDF_PREFILTER" else "plain")


def test_fused_stage_k75(tmp_path, two_stage, ref_jf):
    from kmer_denovo_filter_amd import devkeys
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_non_ref_kmers
    want = two_stage(75)
    assert want[0] > want[1] > 0
    fa, n_cand, n_non_ref = _extract_child_non_ref_kmers(CHILD, None, ref_jf(75), 75, MIN_CHILD, 4, str(tmp_path))
    assert (n_cand, n_non_ref) == want[:2] and _read(fa) == want[2]
    assert not os.path.exists(os.path.join(str(tmp_path), "child_candidates.fa"))
    dev = devkeys.lookup(fa, 75)
    assert dev is not None and tuple(dev[0].shape) == (n_non_ref, 3)


def test_fused_stage_refuses_an_index_of_another_k(tmp_path, ref_jf):
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_non_ref_kmers
    with pytest.raises(RuntimeError, match="ref subtraction"):
        _extract_child_non_ref_kmers(CHILD, None, ref_jf(31), 33, MIN_CHILD, 4, str(tmp_path))


def test_parent_filter_device_join(tmp_path, two_stage, monkeypatch):
    want = two_stage(31)
    src = str(tmp_path / "child_non_ref_kmers.fa")
    with open(src, "wb") as f:
        f.write(want[2])
    assert _records(want[2]) == 6679
    a, b = str(tmp_path / "default"), str(tmp_path / "join")
    os.makedirs(a); os.makedirs(b)
    from kmer_denovo_filter_amd.discovery import pipeline
    default = _parents(src, 31, a, monkeypatch)
    assert pipeline.LAST_PARENT_FILTER == "query"
    monkeypatch.setenv("KDF_DEVICE_JOIN", "1")
    joined = _parents(src, 31, b, monkeypatch)
    assert pipeline.LAST_PARENT_FILTER == "join"
    assert _records(default[1]) == 1513 and default[0] == 630
    assert joined == default
