"""Writes the 4:4:0 fixtures: tests/golden/jpeg/440/s440_q90.jpg (40 x 48, no restart markers), s440_rst.jpg (its twin with a restart
marker every 2 MCUs) and expected_440.npz (per file: Pillow's pixels under the file's name, the coefficients it was written from under
name + '_coef', its quantisation tables under name + '_qt'). Pillow's encoder cannot write this sampling: the files come from
tests/jpeg_440_craft.py -- the transposed coefficient blocks of a 4:2:2 file Pillow wrote, i.e. a losslessly transposed photograph.
They sit in a directory of their own because tests/test_jpeg.py and tests/test_jpeg_gpu.py take every .jpg beside expected.npz for a
file the DEFAULT settings decode.   python -m tests.golden.gen_jpeg_440_fixtures"""
import os

import numpy as np

from tests import jpeg_440_craft as C4
from tests import jpeg_craft as JC

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg', '440')

if __name__ == '__main__':
    os.makedirs(HERE, exist_ok=True)
    coef, qt = C4.picture_coef(90, 40, 48, quality=90)
    exp = {}
    for name, dri in (('s440_q90', 0), ('s440_rst', 2)):
        data = C4.write(40, 48, coef, qt, dri=dri)
        with open(os.path.join(HERE, name + '.jpg'), 'wb') as f:
            f.write(data)
        exp[name], exp[name + '_coef'], exp[name + '_qt'] = JC.pillow(data), coef, qt
        print(name, len(data), 'bytes')
    np.savez_compressed(os.path.join(HERE, 'expected_440.npz'), **exp)
