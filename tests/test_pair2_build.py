"""The two-way pair form of the fused n = 4096 kernels (k_encode_encrypt_pair2, encode_encrypt.hip): its resource plan,
read from the compiler's per-kernel table (tools/resource_usage.py).  No GPU."""
from build_support import resource_rows


def test_pair2_kernel_meets_its_resource_plan():
    """Three workgroups per CU: at most 168 VGPRs and 3 waves per SIMD (its dynamic LDS against three workgroups per CU is
    a static_assert beside the kernel).  The one-plane forms it leaves the keyed, odd and flagged launches to are still
    compiled.
    Scratch: the rule is the one-plane pair form's -- none outside the exact-redo branch.  The kernel as built needs none
    ANYWHERE, which the table shows without reading the ISA, so it is held to zero: stricter than the rule, and a compiler
    that starts to spill in the redo branch makes this fail and the ISA worth a look."""
    rows = resource_rows("encode_encrypt")
    assert len(rows) > 30, rows
    for mode in (0, 2):
        vgpr, scratch, occ = rows[f"k_encode_encrypt_pair2<12, {mode}>"]
        print(f"k_encode_encrypt_pair2<12, {mode}>: {vgpr} VGPRs, {scratch} B scratch, {occ} waves per SIMD")
        assert vgpr <= 168 and occ >= 3, (mode, vgpr, occ)
        assert scratch == 0, (mode, scratch)
    for mode in (0, 1, 2):
        assert f"k_encode_encrypt<12, {mode}>" in rows, mode
