"""The triplet-loss kernels of both models return exactly the recorded bytes.

tests/golden/loss_bits/loss_bits.npz was recorded by tests/golden/gen_loss_bits.py with the library as it stood BEFORE the slab,
batch-hard and partial-sum kernels of cvig_fov and cvig_baseline were folded into one set templated on the term (csrc/loss_kernels.h,
csrc/loss_terms.h): every entry of both models' loss paths, dense and column-slab, soft margin and hinge, with a NaN and +inf in the
batch-hard cases, at shapes that reach every loop of the kernels (see SHAPES there). Equality is by bytes, without a tolerance: a
change to the reduction order, the operation order of a term or the slab indexing shows here for both models.

The fixture depends on the toolchain's device expf / logf. When ROCm changes and this test fails on every soft-margin entry while the
hinge entries still pass, regenerate it with that script (from a library whose kernels are known good) on an MI355X."""
import numpy as np
import pytest

from .golden import gen_loss_bits

pytestmark = pytest.mark.gpu


def test_loss_kernels_return_the_recorded_bits():
    want = np.load(gen_loss_bits.PATH)
    got = gen_loss_bits.outputs()
    assert sorted(got) == sorted(want.files)
    bad = [k for k, a in got.items() if a.dtype != want[k].dtype or a.shape != want[k].shape or a.tobytes() != want[k].tobytes()]
    assert not bad, '%d of %d outputs differ from the recorded bytes: %s' % (len(bad), len(got), bad[:20])
