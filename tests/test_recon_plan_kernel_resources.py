"""Resources of the reconstruction-plan kernels, read from the code objects in libheifhip.so (no GPU needed): k_recon_plan is a streaming kernel and uses no
scratch memory; k_recon8 without the staged unit words and the availability bitmap needs less LDS than the 6072 B it had with them."""
import test_kernel_resources as R


def test_plan_kernel_uses_no_scratch_memory():
    for k in R._find(R._kernels(), "k_recon_plan"):
        assert k["scratch"] == 0


def test_recon8_lds_is_below_what_it_was_with_the_unit_words_and_the_bitmap():
    recon8 = R._find(R._kernels(), "8k_recon8E")[0]
    assert recon8["lds"] < 6072
