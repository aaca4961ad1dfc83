"""Child process of tests/test_gpu_topk_margin.py: the first form of K4's bound-and-refine pass (csrc/topk.hip score_topk_bf16_kernel)
on the adversarial cases of tests/_margin_oracle.py.  TKR_TOPK_V2 and TKR_TOPK_IMAGE are read once per process, so the parent sets
them and starts this script afresh; argv[1] = 1 when the tile image is expected.  Not a test module."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'top-k-rec_amd'), HERE]

import _margin_oracle as M
import tkr_hip


def main():
    image = sys.argv[1] == '1'
    assert os.environ.get('TKR_TOPK_V2') == '0' and (os.environ.get('TKR_TOPK_IMAGE') == '0') == (not image)
    tkr_hip.lib()
    for i, p in enumerate(M.FIRST_FORM_CASES):
        M.run_case_on_gpu(tkr_hip, p, form=1, image=image, via_user_idx=i % 4 == 2)
    # above 65,535 columns: 32-bit ids, user blocks of 192, the work-item table instead of the plain grid
    report = M.run_case_on_gpu(tkr_hip, M.WIDE_ID_CASE, form=1, image=image, id_bits=32, same_range=False)
    assert report['pieces'] > report['blocks']
    print('first form ok: %d cases' % (len(M.FIRST_FORM_CASES) + 1))


if __name__ == '__main__':
    main()
