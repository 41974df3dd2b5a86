"""CPU-side checks of the C-ABI entries of cvig_baseline's bf16 training path: declared, exported, typed, and refusing bad arguments
before any launch (tests/test_abi.py covers the boundary as a whole)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ('witw_conv3x3_bf16_pack_weights_taps4_ex', 'witw_conv3x3_bf16_fwd_taps4_plain', 'witw_space_to_depth2_bf16', 'witw_f32_to_bf16',
           'witw_conv3x3_wgrad_bf16_taps4_workspace_floats', 'witw_conv3x3_wgrad_bf16_taps4')


def test_entries_are_declared_exported_and_typed():
    from witw_amd import _lib
    lib = _lib.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'witw_hip.h')).read(), flags=re.S)
    for n in ENTRIES:
        assert re.search(r'\b%s\s*\(' % n, src), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
        decl = re.search(r'%s\s*\(([^;]*)\)\s*;' % n, src).group(1)
        assert len([a for a in decl.split(',') if a.strip()]) == len(_lib.SIGNATURES[n][1]), n


def test_argument_errors_without_gpu():
    from witw_amd import _lib
    lib = _lib.load()
    err = lambda: lib.witw_last_error()
    # 9 * Cin * Cout floats per split partial (the full-window stride every entry sizes with) + Cout bias floats
    ws = lib.witw_conv3x3_wgrad_bf16_taps4_workspace_floats(1, 8, 16, 16, 8)
    assert ws == 9 * 16 * 8 + 8                                   # one K chunk: one split
    assert lib.witw_conv3x3_wgrad_bf16_taps4_workspace_floats(1, 16, 16, 16, 8) == 2 * (9 * 16 * 8 + 8)
    rc = lib.witw_conv3x3_wgrad_bf16_taps4(None, 1, 1, None, 1, 1, 4, 4, 16, 16, 8, 0, None)
    assert rc == -1 and b'null' in err()
    rc = lib.witw_conv3x3_wgrad_bf16_taps4(1, 1, 1, None, 1, 1, 4, 4, 16, 16, 6, 0, None)
    assert rc == -1 and b'multiples of 4' in err()
    rc = lib.witw_conv3x3_wgrad_bf16_taps4(1, 1, 1, None, 1, 1, 4, 4, 12, 12, 8, 0, None)
    assert rc == -1 and b'multiple of 8' in err()
    rc = lib.witw_conv3x3_wgrad_bf16_taps4(1, 1, 1, None, 1, 1, 4, 4, 16, 17, 8, 0, None)
    assert rc == -1 and b'cin_real' in err()
    rc = lib.witw_conv3x3_bf16_fwd_taps4_plain(1, 1, None, None, 1, 4, 4, 16, 8, 0, 0.0, 1, 4, 4, None)
    assert rc == -1 and b'null' in err()
    rc = lib.witw_conv3x3_bf16_fwd_taps4_plain(1, 1, None, 1, 1, 4, 4, 24, 8, 0, 0.0, 1, 4, 4, None)
    assert rc == -1 and b'multiple of 16' in err()
    rc = lib.witw_conv3x3_bf16_fwd_taps4_plain(1, 1, None, 1, 1, 4, 4, 16, 8, 0, 0.0, 2, 4, 4, None)
    assert rc == -1 and b'tap_base' in err()
    rc = lib.witw_conv3x3_bf16_fwd_taps4_plain(1, 1, None, 1, 1, 4, 4, 16, 8, 0, 0.0, 0, 5, 4, None)
    assert rc == -1 and b'valid region' in err()
    rc = lib.witw_conv3x3_bf16_pack_weights_taps4_ex(None, 1, 8, 16, 1, None)
    assert rc == -1 and b'null' in err()
    rc = lib.witw_conv3x3_bf16_pack_weights_taps4_ex(1, 1, 0, 16, 1, None)
    assert rc == -1 and b'bad shape' in err()
    rc = lib.witw_space_to_depth2_bf16(1, 1, 1, 4, 4, 4, 4, 6, None, None, None)
    assert rc == -1 and b'multiple of 4' in err()
    rc = lib.witw_space_to_depth2_bf16(1, 1, 1, 4, 4, 5, 4, 8, None, None, None)
    assert rc == -1 and b'bad shape' in err()
    rc = lib.witw_space_to_depth2_bf16(1, 1, 1, 4, 4, 4, 4, 8, 1, None, None)
    assert rc == -1 and b'go together' in err()
    rc = lib.witw_f32_to_bf16(1, 1, 0, None)
    assert rc == -1 and b'n <= 0' in err()
