"""CPU: the host-visible pieces of the split-bf16 Winograd weight gradient (csrc/winograd_wgrad4.hip): its three prototypes parse from
include/crb_hip.h with the argument lists of the crb_winograd2_wgrad trio, the built library exports them (and none of its measurement
knobs), and crb_winograd4_wgrad_supported answers for the bench shapes and the shapes the GPU tests use."""
import subprocess


def test_prototypes_match_the_f32_trio():
    import crbhip
    protos = crbhip.parse_header()
    for tail in ('wgrad', 'wgrad_supported', 'wgrad_workspace_bytes'):
        assert 'crb_winograd4_' + tail in protos
        assert protos['crb_winograd4_' + tail] == protos['crb_winograd2_' + tail], tail
    measure = crbhip.parse_header(crbhip._lib.measure_header_path)
    assert 'crb_winograd4_wgrad_set_mode' in measure and 'crb_winograd4_wgrad_set_mode' not in protos


def test_library_exports_the_entry_points_and_no_knob():
    import crbhip
    exported = subprocess.check_output(['nm', '-D', '--defined-only', crbhip.lib_path], text=True)
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    for name in ('crb_winograd4_wgrad', 'crb_winograd4_wgrad_supported', 'crb_winograd4_wgrad_workspace_bytes'):
        assert name in names, name
    assert 'crb_winograd4_wgrad_set_mode' not in names


def test_supported_answers():
    from crbhip import lib
    ok = lib.crb_winograd4_wgrad_supported
    for cin, cout, H, W in ((128, 128, 200, 176), (256, 256, 100, 88), (256, 128, 200, 176),      # the BEV backbone's layers
                            (128, 256, 12, 9), (384, 128, 18, 23), (128, 128, 1, 1), (1024, 1024, 8, 8)):
        assert ok(cin, cout, H, W) == 1, (cin, cout, H, W)
    for cin, cout, H, W in ((64, 64, 50, 44), (64, 192, 7, 5), (192, 128, 10, 10), (128, 64, 40, 31), (128, 96, 10, 10), (0, 128, 4, 4),
                            (2048, 128, 8, 8), (128, 2048, 8, 8), (128, 128, 0, 4)):
        assert ok(cin, cout, H, W) == 0, (cin, cout, H, W)
    # everything the split kernel declines and the f32 kernel takes stays on the f32 kernel
    assert lib.crb_winograd2_wgrad_supported(64, 192, 7, 5) == 1 and lib.crb_winograd2_wgrad_supported(192, 128, 10, 10) == 1
    assert lib.crb_winograd4_wgrad_workspace_bytes(128, 96) == 0
    for cin, cout in ((128, 128), (256, 256), (256, 128)):
        n = lib.crb_winograd4_wgrad_workspace_bytes(cin, cout)
        # a whole number of ranges (a multiple of 8) of 16 x Cin x Cout f32 partials
        assert n > 0 and n % (8 * 16 * cin * cout * 4) == 0, (cin, cout, n)


def test_dispatcher_knob_default():
    import os
    from crbhip import winograd
    assert winograd.WGRAD_KERNEL == os.environ.get('CRB_WINOGRAD_WGRAD_KERNEL', 'x6')
    assert winograd.wgrad_supported(128, 128, 200, 176) and winograd.wgrad_supported(64, 192, 7, 5)
    assert not winograd.wgrad_supported(100, 128, 10, 10)
