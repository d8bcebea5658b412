"""Host only: `expected_kernel` of tests/test_gpu_conv2d_layers.py -- the restatement of the 2-D dispatch of conv_block the
launch-probe assertions of that file rest on -- against the table's own first column in a default process, and against
hand-derived expectations under switches.  Needs neither a GPU nor the library."""
from tests import test_gpu_conv2d_layers as layers
from tests.test_gpu_conv2d_layers import (BOUND, CHAINED, DIRECT, FAMILIES, MB1, MB4, PLAIN, T8, T8W, W4, W6, W16, X3B,
                                          X3F)


def by_kernel(kernel):
    return [c for c in layers.CASES if c[0] == kernel]


def test_default_process_lands_on_the_first_column():
    assert all(layers.expected_kernel(c, {}) == c[0] for c in layers.CASES)
    assert {c[0] for c in layers.CASES} == set(FAMILIES)
    ids = [layers.case_id(c) for c in layers.CASES]
    assert len(set(ids)) == len(ids)


def test_switches_without_the_gate_are_not_seen():
    assert layers.active_switches({'PDS_X3': '0'}) == {}
    assert layers.active_switches({'PDS_X3': '0', 'PDS_DEBUG_SWITCHES': '1'})['PDS_X3'] == '0'


def test_table_reaches_the_forms_and_edges_it_names():
    """The boundaries read off the predicates, each held by a case on either side."""
    shapes = {(c[0], c[1], c[3], c[4], c[6], c[7]) for c in layers.CASES}   # kernel, entry, cin, cout, h, w
    assert (X3B, PLAIN, 256, 64, 9, 20) in shapes and (DIRECT, PLAIN, 260, 64, 5, 10) in shapes
    assert (X3B, PLAIN, 48, 64, 9, 20) in shapes and any(c[0] == W4 and c[3] == 32 for c in layers.CASES)
    assert any(c[0] == X3B and c[1] == CHAINED for c in layers.CASES)
    for kernel, widths in ((T8W, {64, 100, 256, 260, 352}), (T8, {36, 66, 356, 64, 32, 33, 50})):
        assert widths <= {c[7] for c in by_kernel(kernel)}, kernel
    assert {8, 13, 20} <= {c[6] for c in by_kernel(T8W)} and (T8, BOUND, 64, 8, 7, 64) in shapes
    assert all(c[1] == BOUND and not c[10] and (c[3], c[4]) == (64, 8) for c in by_kernel(T8W) + by_kernel(T8))
    assert {1, 5, 13, 8, 16} <= {c[4] for c in by_kernel(MB1)}
    assert {1, 7, 33} <= {c[7] for c in by_kernel(MB4)} and all(c[7] % 2 for c in by_kernel(MB4))
    assert any(c[1] == BOUND and c[10] and (c[3], c[4]) == (64, 8) for c in by_kernel(MB1))
    assert all(c[7] % 4 == 0 for c in by_kernel(W16)) and 4 in {c[7] for c in by_kernel(W16)}
    for kernel in (W4, W6, W16, MB4, MB1, DIRECT):
        assert {PLAIN, CHAINED} <= {c[1] for c in by_kernel(kernel)}, kernel   # with and without a.scale
    # the six-row launches: more than 256 four-row tiles, at most 256 six-row ones
    for c in by_kernel(W6):
        planes, tx = c[2] * c[5], -(-c[7] // 64)
        assert planes * tx * -(-c[6] // 4) > 256 >= planes * tx * -(-c[6] // 6)


def test_wino_rows6_off_keeps_four_row_tiles():
    switches = {'PDS_WINO_ROWS6': '0'}
    for c in layers.CASES:
        assert layers.expected_kernel(c, switches) == (W4 if c[0] == W6 else c[0]), layers.case_id(c)


def test_x3_off_sends_the_64_channel_layers_to_the_exact_kernels():
    """PDS_X3=0: every conv2d_x3 case falls through to conv2d_mfma_supported -- Winograd domain on even widths (16 x 16
    tiles where they are fewer), the direct kernel on odd ones.  Derived by hand from the shapes of the table."""
    want = {             # (h, w): square tiles against wide ones
        (16, 32): W16,   # 1 x 2 = 2 < 4 x 1 = 4
        (17, 33): MB4,   # odd width
        (20, 36): W4,    # 2 x 3 = 6 against 5 x 1 = 5: four-row tiles
        (9, 20): W16,    # 1 x 2 = 2 < 3 x 1 = 3
        (12, 40): W4,    # 1 x 3 = 3 against 3 x 1 = 3: four-row tiles
        (33, 65): MB4,   # odd width
    }
    switches = {'PDS_X3': '0'}
    seen = set()
    for c in by_kernel(X3B) + by_kernel(X3F):
        assert layers.expected_kernel(c, switches) == want[(c[6], c[7])], layers.case_id(c)
        seen.add((c[6], c[7]))
    assert seen == set(want)
    for c in layers.CASES:
        if c[0] not in (X3B, X3F):
            assert layers.expected_kernel(c, switches) == c[0]
    # ... and with PDS_WINOGRAD=0 as well, everything that ran in the Winograd domain takes the direct MFMA kernel
    switches = {'PDS_X3': '0', 'PDS_WINOGRAD': '0'}
    for c in layers.CASES:
        moved = MB4 if c[0] in (X3B, X3F, W4, W6, W16) else c[0]
        assert layers.expected_kernel(c, switches) == moved, layers.case_id(c)
    # PDS_WINO_TILE16=0: the square-tile cases on four-row tiles (none of them is large enough for six rows)
    for c in by_kernel(W16):
        assert layers.expected_kernel(c, {'PDS_WINO_TILE16': '0'}) == W4


def test_t8_switches():
    for c in layers.CASES:
        assert layers.expected_kernel(c, {'PDS_CONV2D_T8W': '0'}) == (T8 if c[0] == T8W else c[0])
        assert layers.expected_kernel(c, {'PDS_CONV2D_T8': '0'}) == (MB1 if c[0] in (T8, T8W) else c[0])
        assert layers.expected_kernel(c, {'PDS_CONV2D_T8W_ROWS': '8'}) == c[0]   # (another instantiation, same family)
        assert layers.expected_kernel(c, {'PDS_X3_FP16': '0'}) == (X3B if c[0] == X3F else c[0])
