"""The benefit scene of the marginalising slide on the reference alone (tests/slide_benefit_ref.py): what tests/test_gpu_slide_marginalize.py
then asks of the device.  Nothing here is tuned: the scene's default seed, the figures as they come."""
from tests import slide_benefit_ref as sb


def test_reference_shows_the_benefit(oracle):
    sc = sb.scene()
    x_plain, p_plain = sb.run_reference(oracle, sc, False)
    x_marg, p_marg = sb.run_reference(oracle, sc, True)
    e_plain, e_marg = sb.errors(sc, x_plain), sb.errors(sc, x_marg)
    print(f"plain |dbg| {e_plain[0]:.6e} |dv| {e_plain[1]:.6e}; marginalising {e_marg[0]:.6e} {e_marg[1]:.6e}")
    assert p_plain is None and p_marg is not None and p_marg["kf"] == sb.N_KF - 2 and p_marg["c0"] >= 0.0
    assert e_marg[0] < e_plain[0] and e_marg[1] < e_plain[1]
    assert e_plain[0] < 0.2 * float((sb.BG_TRUE ** 2).sum() ** 0.5), "both runs find most of the bias step"
