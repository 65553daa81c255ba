"""Resources of the reconstruction kernels with the 16-byte plan records, read from the code objects in libheifhip.so (no GPU needed).  k_recon8 stays on
its occupancy step (7 waves per SIMD by registers: 72 VGPRs; 4800 B of LDS per wave) with no more spill space than it had with the 8-byte records, the
plan kernel stays a streaming kernel without LDS or scratch although it now fills the masks and classes, and k_recon16, which shares the block templates,
keeps its register count and stays free of scratch."""
import test_kernel_resources as R


def test_recon8_keeps_its_occupancy_step_and_its_spill_space():
    recon8 = R._find(R._kernels(), "8k_recon8E")[0]
    print("k_recon8", recon8)
    assert recon8["vgpr"] <= 72
    assert recon8["scratch"] <= 100
    assert recon8["lds"] <= 4800


def test_plan_kernel_uses_neither_scratch_nor_lds():
    for k in R._find(R._kernels(), "k_recon_plan"):
        print("k_recon_plan", k)
        assert k["scratch"] == 0
        assert k["lds"] == 0


def test_recon16_keeps_its_registers_and_uses_no_scratch():
    recon16 = R._find(R._kernels(), "9k_recon16E")[0]
    print("k_recon16", recon16)
    assert recon16["vgpr"] <= 103
    assert recon16["scratch"] == 0
