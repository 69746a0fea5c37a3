"""The GEMM family's selection policy (csrc/gemm.hip, gemm_route) from the host, through the test hook sdxl_debug_gemm_route: no device needed.

tests/golden/gemm_routes.json holds every distinct GEMM problem of one training step of three bench.py workloads (ddpm_b4_1024; ddpm_b1_512: the
small-problem split-K routes; flow_b4_1344x768: ragged tiles) as the launch log describes it, with the kernel family, configuration, staging form and
split-K pass that the library BEFORE gemm_route existed ran for it, read off the kernel names of a rocprofv3 trace (profiles/tools/gemm_route_trace.py,
profiles/gemm_route_trace.txt) -- not off gemm_route's answer."""
import json
from pathlib import Path

import pytest

import sdxl_amd  # noqa: F401
from sdxl_amd import lib

ROWS = json.loads((Path(__file__).parent / "golden" / "gemm_routes.json").read_text())


@pytest.fixture()
def mode():
    """sets the process-global gemm mode for one test, restores the policy afterwards"""
    L = lib.load()
    yield lambda m: lib.check(L.sdxl_set_gemm_mode(m))
    lib.check(L.sdxl_set_gemm_mode(1))


def test_every_problem_of_the_traced_steps_takes_the_kernel_it_took_before():
    assert len(ROWS) > 300 and all(set(r["problem"]) == set(lib.GEMM_DESC_FIELDS) and set(r["route"]) == set(lib.GEMM_ROUTE_FIELDS) for r in ROWS)
    assert {r["route"]["kernel"] for r in ROWS} == {"128-row", "256x256", "cr256", "pipelined", "wgrad256", "conv_wgrad3"}      # all but stream-K
    assert {r["route"]["post"] for r in ROWS} == {"none", "splitk_reduce", "splitk_epilogue"}
    wrong = [(r, got) for r in ROWS if (got := lib.gemm_route(**r["problem"])) != r["route"]]
    assert not wrong, f"{len(wrong)} of {len(ROWS)} problems changed their route; the first: {wrong[0]}"


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("cfg", [3, 13, 23])
def test_forced_160_column_configurations_need_n_divisible_by_160(form, cfg):
    for M, N, K in [(300, 200, 128), (4, 136, 64), (129, 128, 192)]:
        assert lib.gemm_route(form=form, M=M, N=N, K=K, cfg=cfg)["cfg"] == 1
    r = lib.gemm_route(form=form, M=304, N=320, K=128, cfg=cfg)
    assert (r["kernel"], r["cfg"]) == ("128-row", cfg)


@pytest.mark.parametrize("form", [0, 1])
def test_mode_2_takes_the_256x256_kernel_on_whole_tiles_only(form, mode):
    mode(2)
    assert lib.gemm_route(form=form, M=256, N=256, K=128)["kernel"] == "256x256"
    assert lib.gemm_route(form=form, M=512, N=256, K=128)["kernel"] == "256x256"
    assert lib.gemm_route(form=form, M=300, N=256, K=128)["kernel"] == "128-row"
    mode(1)
    assert lib.gemm_route(form=form, M=256, N=256, K=128)["kernel"] == "128-row"      # (one tile: not the policy's)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("cfg", [31, 32])
def test_forced_co_resident_kernel_needs_m_divisible_by_8(form, cfg):
    r = lib.gemm_route(form=form, M=304, N=320, K=128, cfg=cfg)
    assert (r["kernel"], r["cfg"]) == ("cr256", cfg)
    assert lib.gemm_route(form=form, M=4, N=136, K=64, cfg=cfg)["kernel"] == "128-row"      # M % 8
    assert lib.gemm_route(form=form, M=300, N=200, K=128, cfg=cfg)["kernel"] == "128-row"


def test_delta_epilogue_takes_configuration_1_whatever_is_forced(mode):
    for forced in (0, 2, 3, 13, 23, 7, 31, 32):
        for per_launch in (0, 1, 2, 13, 31):
            mode(1 + 4 * forced)
            r = lib.gemm_route(form=1, M=4096, N=1280, K=1280, cfg=per_launch, delta=1)
            assert (r["kernel"], r["cfg"], r["post"]) == ("128-row", 1, "none"), (forced, per_launch, r)
    mode(2)
    assert lib.gemm_route(form=1, M=4096, N=1280, K=1280, delta=1)["kernel"] == "128-row"


def test_the_launch_checks_come_first():
    with pytest.raises(lib.SdxlError, match="multiple of 8"):
        lib.gemm_route(form=0, M=128, N=100, K=64)
    with pytest.raises(lib.SdxlError, match="Delta epilogue"):
        lib.gemm_route(form=0, M=4096, N=1280, K=1280, delta=1)
