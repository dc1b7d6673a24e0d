"""The kernel source of csrc/snpm_k_mos.hpp and the host's slab plan (mos_slab), compiled for the host and run by the real threads of
every block under AddressSanitizer + UBSan (tests/mos_host_driver.cpp on tests/host_kernel/, a stand-alone child process)."""
import host_kernel_util


def test_kernel_source_and_plan_on_the_host_under_asan_and_ubsan(tmp_path):
    """k_win_planes, k_mos_fwd in its four forms and k_mos_back with exact-size heap buffers, arbitrary pad bytes and stale
    workspaces, every state / chain cost / column cost against a per-row transcription of the model: 1 / 2 / 63 / 64 / 65 / 130
    columns and the edges of the forms (255 / 256 / 257: four waves of one column; 1279 / 1280 / 1281: four waves of five columns,
    1281 the widest form of sixteen waves); 1 / 2 / 63 / 64 / 65 / 1023 / 1024 / 1025 rows as one chain and cut at 1 | 63 | 64 | 65;
    several boundaries inside one word, empty chains first, in the middle and last, every row its own chain; S = 1 and 2^20; the
    default table (two cost planes), a random one, all zeros, 15 off the diagonal; column lists with repeats and unsorted row lists
    with a repeat in the three layouts; the split layout at 1135 columns; three slabs of one chain each, samples in groups of two,
    a chain larger than the budget."""
    cases = [ln.split() for ln in host_kernel_util.run_driver("mos_host_driver", tmp_path)]
    assert len(cases) == 41
    widths = [c for c in cases if c[1] == "widths"]
    assert [c[3] for c in widths] == ["acc=%d" % a for a in (1, 2, 63, 64, 65, 130, 255, 256, 257, 1279, 1280, 1281)]
    for rows in (1, 2, 63, 64, 65, 1023, 1024, 1025):
        assert sum(c[5] == "rows=%d" % rows and c[1] in ("rows-one-chain", "rows-chains") for c in cases) == 2, rows
    assert {c[2] for c in cases} == {"layout=0", "layout=1", "layout=2"}
    assert {c[8] for c in cases} >= {"S=1", "S=7", "S=1048576"} and {c[9] for c in cases} == {"table=0", "table=1", "table=2", "table=3"}
    plans = {c[1]: (c[10], c[11]) for c in cases if c[1] in ("three-slabs", "groups-of-two", "chain-over-budget")}
    assert plans == {"three-slabs": ("slabs=3", "groups=3"), "groups-of-two": ("slabs=1", "groups=3"), "chain-over-budget": ("slabs=3", "groups=9")}
