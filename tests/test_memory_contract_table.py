"""CPU side of the memory contract: the case table of tests/test_memory_contract_gpu.py covers every public name of
witw_amd/ops.py that launches a kernel, and the one host path that depends on where a block sits refuses a block that is off its
grid before any kernel is involved."""
import inspect

import numpy as np
import pytest
import torch

from tests import test_memory_contract_gpu as T

# public names of ops.py whose source makes a C-ABI call and that need no contract case
EXCLUDED = {
    # (none: the device JPEG entries live in witw_amd/jpeg.py, not in ops.py; switches and queries such as bf16_wres,
    #  conv_wino, last_kernel_variant or gatebits_dgrad_ok go through _lib.load() without _lib.check and launch nothing)
}


def _launching_names():
    from witw_amd import ops
    names = []
    for name, obj in vars(ops).items():
        if name.startswith('_') or not (inspect.isfunction(obj) or inspect.isclass(obj)) or getattr(obj, '__module__', None) != ops.__name__:
            continue
        if '_lib.check(' in inspect.getsource(obj):
            names.append(name)
    return sorted(names)


def test_every_kernel_launching_entry_has_a_contract_case():
    launching = _launching_names()
    assert len(launching) > 70 and 'conv3x3_fwd' in launching and 'PackedConvBf16' in launching and 'adam_step_multi' in launching
    covered = {e for c in T.CASES for e in c.entries}
    unknown = covered - set(launching)
    assert not unknown, 'the table names entries ops.py does not have: %s' % sorted(unknown)
    missing = [n for n in launching if n not in covered and n not in EXCLUDED]
    assert not missing, 'ops entries that launch a kernel without a memory-contract case: %s' % missing
    assert not set(EXCLUDED) & covered


def test_case_ids_are_unique_and_every_family_is_present():
    ids = [c.id for c in T.CASES]
    assert len(set(ids)) == len(ids)
    assert {c.family for c in T.CASES} >= {'conv_f32', 'conv_f32_wino', 'conv_f32_dgrad', 'first_layer', 'first2_bf16', 'conv_bf16',
                                           'conv_f16x3', 'wgrad', 'pool_bwd', 'layout', 'match', 'loss', 'preprocess', 'baseline', 'adam'}
    assert T.ISOLATION and all(c.skew for c in T.CASES if c.family in ('conv_f32', 'conv_bf16', 'conv_f16x3', 'match', 'loss', 'adam'))


def test_jpeg_part_off_the_128_byte_grid_is_refused_before_any_launch():
    """decode_packed_multi re-bases every part's offsets to the lowest block and addresses tables on a 128-byte grid from there: a
    part 64 bytes off that grid is refused by name instead of decoding with another file's tables. CPU tensors: no kernel runs."""
    from witw_amd import _lib, jpeg
    block = torch.zeros(4096, dtype=torch.uint8)
    base = (-block.data_ptr()) % 128
    a, b = block[base:base + 1024], block[base + 1024 + 64:base + 2048]
    desc = np.zeros((1, 28), dtype=np.int64)
    with pytest.raises(_lib.WitwError, match='part 1 .* 1088 bytes .* not a multiple of 128'):
        jpeg.decode_packed_multi([(a, desc, None), (b, desc, None)])
