"""CEntry of gpu_support (no GPU): the helper the arguments tests of the C entries are written with, on a plain Python
callable in place of a C function."""
import pytest

from gpu_support import SE_ERR_INVALD_ARGUMENT, SE_ERR_NO_KEY, CEntry


def recording(codes):
    """A callable that records its positional arguments and returns the next of `codes`."""
    calls = []

    def fn(*args):
        calls.append(args)
        return codes[len(calls) - 1]

    return fn, calls


def test_edits_land_on_the_named_positions_in_declaration_order():
    fn, calls = recording([0, 0, 0])
    entry = CEntry(fn, ctx="h", c0="p0", B=2, primes=3, stream="s")
    assert entry() == 0 and entry(primes=1) == 0 and entry(stream=None, c0="q") == 0
    assert calls == [("h", "p0", 2, 3, "s"), ("h", "p0", 2, 1, "s"), ("h", "q", 2, 3, None)]
    assert entry.good == dict(ctx="h", c0="p0", B=2, primes=3, stream="s")        # an edit does not stick


def test_an_unknown_field_raises_before_any_call():
    fn, calls = recording([0])
    entry = CEntry(fn, ctx="h", primes=3)
    with pytest.raises(TypeError, match="prime"):
        entry(prime=0)
    with pytest.raises(TypeError, match="prime"):
        entry.refused([dict(prime=0)])
    assert calls == []


def test_refused_names_the_case_that_returned_another_code():
    fn, calls = recording([SE_ERR_INVALD_ARGUMENT, 0, SE_ERR_INVALD_ARGUMENT])
    entry = CEntry(fn, ctx="h", primes=3)
    with pytest.raises(AssertionError) as err:
        entry.refused([dict(ctx=None), dict(primes=4), dict(primes=0)])
    assert "case 1" in str(err.value) and "'primes': 4" in str(err.value) and "returned 0" in str(err.value)
    assert calls == [(None, 3), ("h", 4)]                                         # it stops at the first miss
    fn, calls = recording([SE_ERR_NO_KEY, SE_ERR_NO_KEY])
    CEntry(fn, elt=3).refused([dict(elt=5), {}], SE_ERR_NO_KEY)
    assert calls == [(5,), (3,)]
