"""The operand-isolation helper (tests/_isolation.py) can fail: three fake ops in plain torch on a CPU arena -- a well-behaved one passes,
one that writes into a column gap is caught by the guard check, one that adds a guard row into its result is caught by the bit comparison."""
import pytest
import torch

from _isolation import ALIGN, FILLS, MIN_BAND, Arena, Spec, assert_isolated, run_isolated, same_bits


def _specs(rows=5, cols=16, gap=8):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(rows, cols, generator=g)
    return [Spec("x", rows, cols, cols + gap, torch.bfloat16, x, "in"), Spec("y", rows, cols, cols + gap, torch.float32, None, "out")]


def _good(a):
    a["y"].copy_(a["x"].float() * 2.0 + 1.0)


def test_byte_patterns_mean_what_the_helper_says():
    for dtype in (torch.bfloat16, torch.float32):
        nan, big, zero = (Arena(f).pattern(dtype) for f in (0xFF, 0x7F, 0x00))
        assert bool(torch.isnan(nan)) and float(zero) == 0.0
        assert bool(torch.isfinite(big)) and 3.38e38 < float(big) < 3.40e38
    a = Arena(0xFF)
    a.add(Spec("s", 3, 8, 16, torch.bfloat16, None, "scratch"))
    a.commit()
    assert bool(torch.isnan(a["s"]).all())                 # an operand without contents starts as the pattern


def test_layout_alignment_bands_and_views():
    a = Arena(0x7F)
    for s in _specs(rows=300, cols=200, gap=8):
        a.add(s)
    a.commit()
    for name, isz in (("x", 2), ("y", 4)):
        assert a.ptr(name) % ALIGN == 0 and a.ld(name) == 208
        assert a[name].shape == (300, 200) and a[name].stride() == (208, 1) and a[name].data_ptr() == a.ptr(name)
    band_x, band_y = max(256 * 208 * 2, MIN_BAND), max(256 * 208 * 4, MIN_BAND)
    assert a.off["x"] >= band_x and a.off["y"] - (a.off["x"] + 300 * 208 * 2) >= band_x + band_y
    assert a.buf.numel() - (a.off["y"] + 300 * 208 * 4) >= band_y
    # guard = every byte that is no operand element: the column gaps included
    assert int((~a.guard).sum()) == 300 * 200 * (2 + 4)
    assert bool(a.guard[a.off["x"] + 200 * 2: a.off["x"] + 208 * 2].all()) and not bool(a.guard[a.off["x"] + 199 * 2])
    assert same_bits(a["x"], _specs(300, 200)[0].init.to(torch.bfloat16))


def test_well_behaved_op_passes():
    runs = run_isolated(_good, _specs())
    assert len(runs) == len(FILLS) and set(runs[0]) == {"y"}
    assert_isolated(runs)
    assert torch.equal(runs[0]["y"], _specs()[0].init.to(torch.bfloat16).float() * 2.0 + 1.0)


def test_write_into_a_column_gap_is_caught():
    def op(a):
        _good(a)
        s = a.spec("y")
        a.buf[a.off["y"]: a.off["y"] + s.rows * s.ld * 4].view(torch.float32).view(s.rows, s.ld)[2, s.cols] = 1.5     # one element past N
    with pytest.raises(AssertionError, match=r"guard byte written.*operand 'y'.*row 2, byte 6[4-7] of the row"):
        run_isolated(op, _specs())


def test_write_behind_the_last_row_and_into_an_input_are_caught():
    def past_end(a):
        _good(a)
        s = a.spec("y")
        a.buf[a.off["y"] + s.rows * s.ld * 4 + 12] = 1
    with pytest.raises(AssertionError, match=r"guard byte written.*operand 'y'.*behind its last"):
        run_isolated(past_end, _specs())

    def clobber(a):
        _good(a)
        a["x"][1, 3] = 7.0
    with pytest.raises(AssertionError, match=r"read-only operand written.*operand 'x'.*row 1"):
        run_isolated(clobber, _specs())


def test_read_of_a_guard_row_is_caught_by_the_bit_comparison():
    def op(a):
        s = a.spec("x")
        past = a.buf[a.off["x"]: a.off["x"] + (s.rows + 1) * s.ld * 2].view(torch.bfloat16).view(s.rows + 1, s.ld)[s.rows, : s.cols]   # the row behind M
        a["y"].copy_(a["x"].float() * 2.0 + 1.0)
        a["y"][s.rows - 1] += 0.0 * past.float()           # 0 * NaN: the classic masked-by-multiplication leak
        a["y"][0] = torch.maximum(a["y"][0], past.float() * 1e-38)      # a comparison swallows NaN, not 3.39e38
    runs = run_isolated(op, _specs())                      # guards and inputs are untouched: only the results tell
    with pytest.raises(AssertionError, match=r"fill 0xFF: output 'y' is not finite"):
        assert_isolated(runs)
    with pytest.raises(AssertionError, match=r"fill 0x7F: output 'y' differs from the clean run"):
        assert_isolated([runs[0], runs[2]], fills=(0x00, 0x7F))


def test_cross_row_form_poisons_only_the_named_rows():
    def rowwise(a):
        a["y"].copy_(a["x"].float().cumsum(1))

    def leaky(a):
        a["y"].copy_(a["x"].float().cumsum(1) + 0.0 * a["x"].float().sum(0, keepdim=True))
    keep = {"y": slice(0, 3)}
    assert_isolated(run_isolated(rowwise, _specs(), poison={"x": slice(3, 5)}), rows=keep)
    with pytest.raises(AssertionError, match="fill 0xFF"):
        assert_isolated(run_isolated(leaky, _specs(), poison={"x": slice(3, 5)}), rows=keep)


def test_atomic_outputs_get_the_relative_bar_and_nothing_more():
    y = torch.ones(4, 8)
    runs = [{"y": y}, {"y": y * (1 + 5e-6)}, {"y": y}]
    assert_isolated(runs, atomic=("y",))
    with pytest.raises(AssertionError):
        assert_isolated(runs)
    with pytest.raises(AssertionError, match="moved by"):
        assert_isolated([{"y": y}, {"y": y * (1 + 5e-5)}], fills=(0x00, 0xFF), atomic=("y",))
