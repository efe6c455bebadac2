"""CPU-side check of what kernels/ct_ops.hip compiles to for gfx950: the set of kernels and each kernel's scratch, waves
per SIMD and registers against the one table of tests/ct_ops_resources.py.  Any edit to device code the kernels share can
move any of them, so each test collects every offender and asserts once (no GPU needed)."""
from build_support import resource_rows
from ct_ops_resources import KERNELS


def built():
    rows = resource_rows("ct_ops")
    assert rows, "tools/resource_usage.py gave no table for ct_ops"
    return rows


def test_compiled_kernels_are_the_tables_kernels():
    """Nothing went missing and nothing is unlisted: a new kernel gets a row in tests/ct_ops_resources.py."""
    rows = built()
    missing, unlisted = sorted(set(KERNELS) - set(rows)), sorted(set(rows) - set(KERNELS))
    assert not missing and not unlisted, f"missing from the build: {missing}; not in the table: {unlisted}"


def test_kernels_keep_their_scratch_waves_and_registers():
    rows = built()
    ok = {"==": lambda a, b: a == b, ">=": lambda a, b: a >= b}
    bad = []
    for k, rule in KERNELS.items():
        if k not in rows:
            continue                                   # test_compiled_kernels_are_the_tables_kernels names it
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD")
        op, n = rule.get("waves", (">=", 0))
        if scratch != rule["scratch"] or not ok[op](occ, n) or vgpr != rule.get("vgprs", vgpr):
            bad.append(f"{k}: built {rows[k]}, rule {rule}")
    assert not bad, "(VGPRs, scratch bytes, waves per SIMD) against the rule:\n" + "\n".join(bad)


def test_kernels_keep_at_least_their_siblings_waves():
    rows = built()
    unknown = [(k, s) for k, rule in KERNELS.items() for s in rule.get("at_least", ()) if s not in KERNELS]
    assert not unknown, f"siblings that are no row of the table: {unknown}"
    bad = []
    for k, rule in KERNELS.items():
        for sibling in rule.get("at_least", ()):
            if k in rows and sibling in rows and rows[k][2] < rows[sibling][2]:
                bad.append(f"{k}: built {rows[k]}, rule at least {sibling}: built {rows[sibling]}")
    assert not bad, "fewer waves per SIMD than a sibling of the same report:\n" + "\n".join(bad)
