"""genotype_cross_hmm on the device: ``snpm_cross_hmm`` / ``k_ghmm`` against the reference's goldens (states and every omega bit)
and, on random inputs at the shapes where the kernel's decomposition (one lane per chain, 64 samples per wave, table loads
GH_UNROLL = 8 steps ahead) could break, against the numpy twin (tests/ghmm_twin.py); then the command line on a flat panel."""
import numpy as np
import pytest

import ghmm_twin
import ghmm_util
from snpmatch_amd import cli, engine
from snpmatch_amd.core import infer, snp_genotype

pytestmark = pytest.mark.gpu
UNROLL = 8


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _same(got_state, got_omega, want_state, want_omega):
    assert np.array_equal(got_state, want_state)
    assert np.array_equal(got_omega.view(np.uint64), want_omega.view(np.uint64))


@pytest.mark.parametrize("name", ghmm_util.CASES)
def test_goldens_through_the_device_call(name, ctx, tmp_path, monkeypatch):
    case = ghmm_util.load(name)
    seen = {}

    def step(*args):
        seen["state"], seen["omega"] = engine.cross_hmm(ctx, *args, return_omega=True)
        return seen["state"]

    lines = ghmm_util.golden_lines(case, monkeypatch, tmp_path, step)
    _same(seen["state"], seen["omega"], case["state"], case["omega"])
    assert lines.tolist() == case["lines"].tolist()


def _run(ctx, case, n_samples):
    codes, rank, pair, off, logT, logI, logE, want_state, want_omega = case
    view, rview = codes[:, :n_samples], rank[:, :n_samples]           # ld = n_samples + 5: the columns behind hold 0xEE / 0xEEEE
    state, omega = engine.cross_hmm(ctx, view, rview, pair, off, logT, logI, logE, return_omega=True)
    _same(state, omega, want_state, want_omega)
    assert np.array_equal(engine.cross_hmm(ctx, view, rview, pair, off, logT, logI, logE), want_state)      # omega == NULL: the same states


# chains of 1, 2, 3 markers, the unroll depth - 1 / + 0 / + 1 (steps: one more marker), 700, empty chains first, inside and last
SIZES = (0, 1, 2, 3, 0, 0, UNROLL - 1, UNROLL, UNROLL + 1, UNROLL + 2, 700, 2 * UNROLL + 1, 0)


@pytest.mark.parametrize("n_samples", [1, 63, 64, 65, 257])
def test_random_chains_against_the_twin(n_samples, ctx):
    case = ghmm_util.random_case(n_samples, SIZES)
    assert len(np.unique(case[7])) == 3
    _run(ctx, case, n_samples)


@pytest.mark.parametrize("sizes", [(40,), (5, 0, 9, 1, 30, 2, 17)], ids=["1-chain", "7-chains"])
@pytest.mark.parametrize("n_depth", [1, 300])
def test_chain_and_depth_counts(sizes, n_depth, ctx):
    _run(ctx, ghmm_util.random_case(70, sizes, n_depth=n_depth), 70)


def test_a_table_holding_minus_infinity(ctx):
    case = ghmm_util.random_case(66, (0, 25, 1, 12, 33), minus_inf=True)
    assert np.isneginf(case[4]).any() and np.isneginf(case[8]).any()   # impossible transitions: -inf reaches omega
    _run(ctx, case, 66)


def test_all_na_chain_ties_resolve_to_the_first_state(ctx):
    """never-called samples: every emission is 1, AA and BB tie exactly at every step; np.argmax takes the first"""
    n, ns = 21, 3
    codes = np.full((n, ns), 3, dtype=np.uint8)                       # './.' everywhere
    rank = np.zeros((n, ns), dtype=np.uint16)
    _, logI, logE = infer.emission_tables([2.0], 0.036)
    logT = infer.log_transition(infer._transition_frame(1.0, n, 3.5).values)[None]
    pair = np.arange(n, dtype=np.uint8) % 6
    want_state, want_omega = ghmm_twin.cross_hmm(codes, rank, pair, [0, n], logT, logI, logE)
    assert np.array_equal(want_omega[:, :, 0], want_omega[:, :, 2])
    state, omega = engine.cross_hmm(ctx, codes, rank, pair, [0, n], logT, logI, logE, return_omega=True)
    _same(state, omega, want_state, want_omega)
    # with every transition impossible all three candidates are -inf from the second marker on: state 0 by the first-maximum rule
    dead = np.full((1, 3, 3), -np.inf)
    want_state, want_omega = ghmm_twin.cross_hmm(codes, rank, pair, [0, n], dead, logI, logE)
    assert np.all(np.isneginf(want_omega[1:])) and np.all(want_state == 0)
    state, omega = engine.cross_hmm(ctx, codes, rank, pair, [0, n], dead, logI, logE, return_omega=True)
    _same(state, omega, want_state, want_omega)


def test_separator_is_governed_by_each_chains_first_row(ctx):
    """one sample, two chains: the first opens with '0/1' (the '|' calls read as 0/0), the second with '1|1' (the '/' calls do)"""
    from snpmatch_amd.core import parsers
    col = ["0/1", "1|1", "1/1", "0|1", "./.", "1|1", "1/1", "0|1", "1|0", "0/1", ".|."]
    codes = parsers.gt_call_codes(np.array([col]).T)
    off = [0, 5, 11]
    obs = ghmm_twin.observations(codes, off)[:, 0].tolist()
    assert obs == [1, 0, 2, 0, 3, 2, 0, 1, 1, 0, 3]
    rank = np.zeros((11, 1), dtype=np.uint16)
    _, logI, logE = infer.emission_tables([3.0], 0.036)
    logT = np.stack([infer.log_transition(infer._transition_frame(1.0, k, 3.5).values) for k in (5, 6)])
    pair = np.zeros(11, dtype=np.uint8)
    want = ghmm_twin.cross_hmm(codes, rank, pair, off, logT, logI, logE)
    got = engine.cross_hmm(ctx, codes, rank, pair, off, logT, logI, logE, return_omega=True)
    _same(got[0], got[1], want[0], want[1])
    # the model class through the same kernel: one chain, the reference's surface
    p1, p2 = np.zeros(5, dtype=np.int8), np.ones(5, dtype=np.int8)
    model = infer.IdentifyAncestryF2individual(1.0, p1, p2, recomb_rate=3.5, base_error=0.036, sample_depth=np.repeat(3.0, 5))
    path, omega = model.viterbi(parsers.parseGT(np.array(col[:5])))
    assert path.dtype == float and np.array_equal(path, want[0][:5, 0]) and np.array_equal(omega.view(np.uint64), want[1][:5, 0].view(np.uint64))


def test_two_sizes_on_one_context_then_destroy():
    own = engine.Context()
    small = ghmm_util.random_case(5, (3, 9))
    large = ghmm_util.random_case(130, (60, 0, 41), n_depth=12)
    for case, ns in ((small, 5), (large, 130), (small, 5)):           # the workspaces grow, then serve the smaller call again
        _run(own, case, ns)
    own.close()


def test_command_line_writes_the_reference_file(tmp_path):
    case = ghmm_util.load("ghmm_a_f2")
    db = str(tmp_path / "db.snpm")
    snp_genotype.save_native(db, case["panel"], case["accessions"], case["positions"], case["chrs"], case["chr_regions"])
    vcf = ghmm_util.write_vcf(str(tmp_path / "f2.vcf"), case["vcf_chr"], case["vcf_pos"], case["vcf_gt"], case["vcf_dp"], case["samples"])
    out = str(tmp_path / "out.csv")
    rc = cli.main(["genotype_cross_hmm", "-i", vcf, "-d", db, "-p", str(case["parents"]),
                   "--genome", ghmm_util.write_genome(case, str(tmp_path / "genome.json")), "-o", out])
    assert rc == 0
    assert open(out).read() == "".join(ln + "\n" for ln in case["lines"].tolist())
