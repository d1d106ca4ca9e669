"""The kernel selection (csrc/fbs_select.cpp) without a GPU: the harness of tests/c, built with -fsanitize=address,undefined as
for tests/test_sanitizers.py, in its `select` mode -- parameter set, CU count, batch size and launcher knobs in; the launches a key
switch and a blind rotation make out, one per line (kind, kernel name, first bootstrap, count).

* every entry of fbs_kernel_catalog is what the selection picks for its recipe (tests/helpers.py) -- the statement
  tests/test_gpu_dispatch.py makes on the GPU, on every CPU run;
* the launches at the boundaries of every family, for the shipped sets and the knobs the tests use: 1, cus, cus + 1, 2 cus,
  2 cus + 1, 3 cus, a round, a round plus a small, a near-full and the largest rest that is still cut off, 8 cus + 60 (a table
  taken from the launchers of the parent commit; the cut points named in the selection's comments are in it: k = 3 at N = 512
  1 024 = 768 + 256, k = 2 at N = 1024 1 124 = 1 024 + 100);
* parameter admission: what fbs_ctx_create refuses the harness refuses with the same code, and out-of-range gadget bases are
  refused before anything is computed from them (no UBSan report)."""
import re
import subprocess

import pytest

from tests.helpers import CUS, recipe
from tests.test_sanitizers import ENV, harness  # noqa: F401  (the same sanitizer build)

# (label, harness parameters "n log_n k l beta t gamma p group", knobs, kind of launch, {count: its launches -- one name, or
# "name*count + name*count" for a launch cut into whole rounds and a rest})
BOUNDARIES = [
    ('P1024', '630 10 1 3 7 8 2 7 1', '', 'br', {
        1: 'k_blind_rotate_cu<10,3,2>', 256: 'k_blind_rotate_cu<10,3,2>', 257: 'k_blind_rotate_cu<10,3,2,lean>',
        512: 'k_blind_rotate_cu<10,3,2,lean>', 513: 'k_blind_rotate<10,6,3,1>', 768: 'k_blind_rotate<10,6,3,1>',
        769: 'k_blind_rotate<10,6,3,1>', 1024: 'k_blind_rotate<10,6,3,4>',
        1124: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2>*100',
        1280: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2>*256',
        1281: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2,lean>*257',
        1536: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2,lean>*512',
        1537: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*513',
        1792: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*768',
        1793: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*769',
        1919: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*895', 1920: 'k_blind_rotate<10,6,3,4>',
        2032: 'k_blind_rotate<10,6,3,4>', 2108: 'k_blind_rotate<10,6,3,4>*2048 + k_blind_rotate_cu<10,3,2>*60',
    }),
    ('P1024 br_cu_kernel=0', '630 10 1 3 7 8 2 7 1', 'br_cu_kernel=0', 'br', {
        1: 'k_blind_rotate<10,8,3,1>', 256: 'k_blind_rotate<10,8,3,1>', 257: 'k_blind_rotate<10,6,3,2>',
        512: 'k_blind_rotate<10,6,3,2>', 513: 'k_blind_rotate<10,6,3,1>', 768: 'k_blind_rotate<10,6,3,1>',
        769: 'k_blind_rotate<10,6,3,1>', 1024: 'k_blind_rotate<10,6,3,4>',
        1124: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,8,3,1>*100',
        1280: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,8,3,1>*256',
        1281: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,2>*257',
        1536: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,2>*512',
        1537: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*513',
        1792: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*768',
        1793: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*769',
        1919: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*895', 1920: 'k_blind_rotate<10,6,3,4>',
        2032: 'k_blind_rotate<10,6,3,4>', 2108: 'k_blind_rotate<10,6,3,4>*2048 + k_blind_rotate<10,8,3,1>*60',
    }),
    ('P1024 br_cu_lean=0', '630 10 1 3 7 8 2 7 1', 'br_cu_lean=0', 'br', {
        1: 'k_blind_rotate_cu<10,3,2>', 256: 'k_blind_rotate_cu<10,3,2>', 257: 'k_blind_rotate_cu<10,3,2>',
        512: 'k_blind_rotate_cu<10,3,2>', 513: 'k_blind_rotate<10,6,3,1>', 768: 'k_blind_rotate<10,6,3,1>',
        769: 'k_blind_rotate<10,6,3,1>', 1024: 'k_blind_rotate<10,6,3,4>',
        1124: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2>*100',
        1280: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2>*256',
        1281: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2>*257',
        1536: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2>*512',
        1537: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*513',
        1792: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*768',
        1793: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*769',
        1919: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*895', 1920: 'k_blind_rotate<10,6,3,4>',
        2032: 'k_blind_rotate<10,6,3,4>', 2108: 'k_blind_rotate<10,6,3,4>*2048 + k_blind_rotate_cu<10,3,2>*60',
    }),
    ('P1024 br_cu_lean=2', '630 10 1 3 7 8 2 7 1', 'br_cu_lean=2', 'br', {
        1: 'k_blind_rotate_cu<10,3,2,lean>', 256: 'k_blind_rotate_cu<10,3,2,lean>', 257: 'k_blind_rotate_cu<10,3,2,lean>',
        512: 'k_blind_rotate_cu<10,3,2,lean>', 513: 'k_blind_rotate<10,6,3,1>', 768: 'k_blind_rotate<10,6,3,1>',
        769: 'k_blind_rotate<10,6,3,1>', 1024: 'k_blind_rotate<10,6,3,4>',
        1124: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2,lean>*100',
        1280: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2,lean>*256',
        1281: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2,lean>*257',
        1536: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate_cu<10,3,2,lean>*512',
        1537: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*513',
        1792: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*768',
        1793: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*769',
        1919: 'k_blind_rotate<10,6,3,4>*1024 + k_blind_rotate<10,6,3,1>*895', 1920: 'k_blind_rotate<10,6,3,4>',
        2032: 'k_blind_rotate<10,6,3,4>', 2108: 'k_blind_rotate<10,6,3,4>*2048 + k_blind_rotate_cu<10,3,2,lean>*60',
    }),
    ('P2048', '630 11 1 3 8 8 2 7 1', '', 'br', {
        1: 'k_blind_rotate<11,8,2,1>', 256: 'k_blind_rotate<11,8,2,1>', 257: 'k_blind_rotate<11,7,2,1>',
        512: 'k_blind_rotate<11,7,2,1>', 513: 'k_blind_rotate<11,7,2,1>', 768: 'k_blind_rotate<11,7,2,1>',
        769: 'k_blind_rotate<11,7,2,1>', 1024: 'k_blind_rotate<11,7,2,1>', 1124: 'k_blind_rotate<11,7,2,1>',
        1280: 'k_blind_rotate<11,7,2,1>', 1281: 'k_blind_rotate<11,7,2,1>', 1536: 'k_blind_rotate<11,7,2,1>',
        1537: 'k_blind_rotate<11,7,2,1>', 1792: 'k_blind_rotate<11,7,2,1>', 1793: 'k_blind_rotate<11,7,2,1>',
        1919: 'k_blind_rotate<11,7,2,1>', 1920: 'k_blind_rotate<11,7,2,1>', 2032: 'k_blind_rotate<11,7,2,1>',
        2108: 'k_blind_rotate<11,7,2,1>',
    }),
    ('N1024 l=2 beta=8', '630 10 1 2 8 8 2 4 1', '', 'br', {
        1: 'k_blind_rotate_cu<10,2,1>', 256: 'k_blind_rotate_cu<10,2,1>', 257: 'k_blind_rotate_cu<10,2,1,lean>',
        512: 'k_blind_rotate_cu<10,2,1,lean>', 513: 'k_blind_rotate<10,6,6,1>', 768: 'k_blind_rotate<10,6,6,1>',
        769: 'k_blind_rotate<10,6,6,1>', 1024: 'k_blind_rotate<10,6,6,1>', 1124: 'k_blind_rotate<10,6,6,1>',
        1280: 'k_blind_rotate<10,6,6,1>', 1281: 'k_blind_rotate<10,6,6,1>', 1536: 'k_blind_rotate<10,6,6,1>',
        1537: 'k_blind_rotate<10,6,6,1>', 1792: 'k_blind_rotate<10,6,6,1>', 1793: 'k_blind_rotate<10,6,6,1>',
        1919: 'k_blind_rotate<10,6,6,1>', 1920: 'k_blind_rotate<10,6,6,1>', 2032: 'k_blind_rotate<10,6,6,1>',
        2108: 'k_blind_rotate<10,6,6,1,false>',
    }),
    ('N2048 l=1 t=14 gamma=1', '718 11 1 1 21 14 1 15 1', '', 'br', {
        1: 'k_blind_rotate_cu<11,1,0>', 256: 'k_blind_rotate_cu<11,1,0>', 257: 'k_blind_rotate_cu<11,1,0>',
        512: 'k_blind_rotate_cu<11,1,0>', 513: 'k_blind_rotate<11,7,4,1>', 768: 'k_blind_rotate<11,7,4,1>',
        769: 'k_blind_rotate<11,7,4,1>', 1024: 'k_blind_rotate<11,7,4,1>', 1124: 'k_blind_rotate<11,7,4,1>',
        1280: 'k_blind_rotate<11,7,4,1>', 1281: 'k_blind_rotate<11,7,4,1>', 1536: 'k_blind_rotate<11,7,4,1>',
        1537: 'k_blind_rotate<11,7,4,1>', 1792: 'k_blind_rotate<11,7,4,1>', 1793: 'k_blind_rotate<11,7,4,1>',
        1919: 'k_blind_rotate<11,7,4,1>', 1920: 'k_blind_rotate<11,7,4,1>', 2032: 'k_blind_rotate<11,7,4,1>',
        2108: 'k_blind_rotate<11,7,4,1>',
    }),
    ('N2048 l=1 two bits', '770 11 1 1 20 8 2 31 2', '', 'br', {
        1: 'k_blind_rotate_cu_pairs<11,1>', 256: 'k_blind_rotate_cu_pairs<11,1>', 257: 'k_blind_rotate_pairs<11,7,4>',
        512: 'k_blind_rotate_pairs<11,7,4>', 513: 'k_blind_rotate_pairs<11,7,4>', 768: 'k_blind_rotate_pairs<11,7,4>',
        769: 'k_blind_rotate_pairs<11,7,4>', 1024: 'k_blind_rotate_pairs<11,7,4>', 1124: 'k_blind_rotate_pairs<11,7,4>',
        1280: 'k_blind_rotate_pairs<11,7,4>', 1281: 'k_blind_rotate_pairs<11,7,4>', 1536: 'k_blind_rotate_pairs<11,7,4>',
        1537: 'k_blind_rotate_pairs<11,7,4>', 1792: 'k_blind_rotate_pairs<11,7,4>', 1793: 'k_blind_rotate_pairs<11,7,4>',
        1919: 'k_blind_rotate_pairs<11,7,4>', 1920: 'k_blind_rotate_pairs<11,7,4>', 2032: 'k_blind_rotate_pairs<11,7,4>',
        2108: 'k_blind_rotate_pairs<11,7,4>',
    }),
    ('N2048 l=2 two bits', '766 11 1 2 13 8 2 31 2', '', 'br', {
        1: 'k_blind_rotate_cu_pairs<11,2>', 256: 'k_blind_rotate_cu_pairs<11,2>', 257: 'k_blind_rotate_cu_pairs<11,2>',
        512: 'k_blind_rotate_cu_pairs<11,2>', 513: 'k_blind_rotate_cu_pairs<11,2>', 768: 'k_blind_rotate_cu_pairs<11,2>',
        769: 'k_blind_rotate_cu_pairs<11,2>', 1024: 'k_blind_rotate_cu_pairs<11,2>', 1124: 'k_blind_rotate_cu_pairs<11,2>',
        1280: 'k_blind_rotate_cu_pairs<11,2>', 1281: 'k_blind_rotate_cu_pairs<11,2>', 1536: 'k_blind_rotate_cu_pairs<11,2>',
        1537: 'k_blind_rotate_cu_pairs<11,2>', 1792: 'k_blind_rotate_cu_pairs<11,2>', 1793: 'k_blind_rotate_cu_pairs<11,2>',
        1919: 'k_blind_rotate_cu_pairs<11,2>', 1920: 'k_blind_rotate_cu_pairs<11,2>', 2032: 'k_blind_rotate_cu_pairs<11,2>',
        2108: 'k_blind_rotate_cu_pairs<11,2>',
    }),
    ('N2048 l=2 two bits br_cu_kernel=0', '766 11 1 2 13 8 2 31 2', 'br_cu_kernel=0', 'br', {
        1: 'k_blind_rotate_pairs<11,7,0>', 256: 'k_blind_rotate_pairs<11,7,0>', 257: 'k_blind_rotate_pairs<11,7,0>',
        512: 'k_blind_rotate_pairs<11,7,0>', 513: 'k_blind_rotate_pairs<11,7,0>', 768: 'k_blind_rotate_pairs<11,7,0>',
        769: 'k_blind_rotate_pairs<11,7,0>', 1024: 'k_blind_rotate_pairs<11,7,0>', 1124: 'k_blind_rotate_pairs<11,7,0>',
        1280: 'k_blind_rotate_pairs<11,7,0>', 1281: 'k_blind_rotate_pairs<11,7,0>', 1536: 'k_blind_rotate_pairs<11,7,0>',
        1537: 'k_blind_rotate_pairs<11,7,0>', 1792: 'k_blind_rotate_pairs<11,7,0>', 1793: 'k_blind_rotate_pairs<11,7,0>',
        1919: 'k_blind_rotate_pairs<11,7,0>', 1920: 'k_blind_rotate_pairs<11,7,0>', 2032: 'k_blind_rotate_pairs<11,7,0>',
        2108: 'k_blind_rotate_pairs<11,7,0>',
    }),
    ('k=2 N1024', '734 10 2 1 21 7 2 15 2', '', 'br', {
        1: 'k_blind_rotate_cu_k2', 256: 'k_blind_rotate_cu_k2', 257: 'k_blind_rotate_cu_k2', 512: 'k_blind_rotate_cu_k2',
        513: 'k_blind_rotate_cu_k2', 768: 'k_blind_rotate_cu_k2', 769: 'k_blind_rotate_pairs_k2<10,4>',
        1024: 'k_blind_rotate_pairs_k2<10,4>', 1124: 'k_blind_rotate_pairs_k2<10,4>*1024 + k_blind_rotate_cu_k2*100',
        1280: 'k_blind_rotate_pairs_k2<10,4>*1024 + k_blind_rotate_cu_k2*256',
        1281: 'k_blind_rotate_pairs_k2<10,4>*1024 + k_blind_rotate_cu_k2*257',
        1536: 'k_blind_rotate_pairs_k2<10,4>*1024 + k_blind_rotate_cu_k2*512',
        1537: 'k_blind_rotate_pairs_k2<10,4>*1024 + k_blind_rotate_cu_k2*513',
        1792: 'k_blind_rotate_pairs_k2<10,4>*1024 + k_blind_rotate_cu_k2*768', 1793: 'k_blind_rotate_pairs_k2<10,4>',
        1919: 'k_blind_rotate_pairs_k2<10,4>', 1920: 'k_blind_rotate_pairs_k2<10,4>', 2032: 'k_blind_rotate_pairs_k2<10,4>',
        2108: 'k_blind_rotate_pairs_k2<10,4>*2048 + k_blind_rotate_cu_k2*60',
    }),
    ('k=2 N1024 br_k2_shape=3', '734 10 2 1 21 7 2 15 2', 'br_k2_shape=3', 'br', {
        1: 'k_blind_rotate_pairs_k2<10,1>', 256: 'k_blind_rotate_pairs_k2<10,1>', 257: 'k_blind_rotate_pairs_k2<10,2>',
        512: 'k_blind_rotate_pairs_k2<10,2>', 513: 'k_blind_rotate_pairs_k2<10,4>', 768: 'k_blind_rotate_pairs_k2<10,4>',
        769: 'k_blind_rotate_pairs_k2<10,4>', 1024: 'k_blind_rotate_pairs_k2<10,4>', 1124: 'k_blind_rotate_pairs_k2<10,4>',
        1280: 'k_blind_rotate_pairs_k2<10,4>', 1281: 'k_blind_rotate_pairs_k2<10,4>', 1536: 'k_blind_rotate_pairs_k2<10,4>',
        1537: 'k_blind_rotate_pairs_k2<10,4>', 1792: 'k_blind_rotate_pairs_k2<10,4>', 1793: 'k_blind_rotate_pairs_k2<10,4>',
        1919: 'k_blind_rotate_pairs_k2<10,4>', 1920: 'k_blind_rotate_pairs_k2<10,4>', 2032: 'k_blind_rotate_pairs_k2<10,4>',
        2108: 'k_blind_rotate_pairs_k2<10,4>',
    }),
    ('k=2 N1024 br_k2_shape=12', '734 10 2 1 21 7 2 15 2', 'br_k2_shape=12', 'br', {
        1: 'k_blind_rotate_cu_k2', 256: 'k_blind_rotate_cu_k2', 257: 'k_blind_rotate_cu_k2', 512: 'k_blind_rotate_cu_k2',
        513: 'k_blind_rotate_cu_k2', 768: 'k_blind_rotate_cu_k2', 769: 'k_blind_rotate_cu_k2', 1024: 'k_blind_rotate_cu_k2',
        1124: 'k_blind_rotate_cu_k2', 1280: 'k_blind_rotate_cu_k2', 1281: 'k_blind_rotate_cu_k2',
        1536: 'k_blind_rotate_cu_k2', 1537: 'k_blind_rotate_cu_k2', 1792: 'k_blind_rotate_cu_k2',
        1793: 'k_blind_rotate_cu_k2', 1919: 'k_blind_rotate_cu_k2', 1920: 'k_blind_rotate_cu_k2',
        2032: 'k_blind_rotate_cu_k2', 2108: 'k_blind_rotate_cu_k2',
    }),
    ('k=3 N512', '670 9 3 1 18 6 2 7 2', '', 'br', {
        1: 'k_blind_rotate_glwe<9,4,2,1>', 256: 'k_blind_rotate_glwe<9,4,2,1>', 257: 'k_blind_rotate_glwe<9,4,2,2>',
        512: 'k_blind_rotate_glwe<9,4,2,2>', 513: 'k_blind_rotate_glwe<9,4,2,3>', 768: 'k_blind_rotate_glwe<9,4,2,3>',
        769: 'k_blind_rotate_glwe<9,4,2,3>*768 + k_blind_rotate_glwe<9,4,2,1>*1',
        868: 'k_blind_rotate_glwe<9,4,2,3>*768 + k_blind_rotate_glwe<9,4,2,1>*100',
        1024: 'k_blind_rotate_glwe<9,4,2,3>*768 + k_blind_rotate_glwe<9,4,2,1>*256',
        1025: 'k_blind_rotate_glwe<9,4,2,3>*768 + k_blind_rotate_glwe<9,4,2,2>*257',
        1280: 'k_blind_rotate_glwe<9,4,2,3>*768 + k_blind_rotate_glwe<9,4,2,2>*512', 1281: 'k_blind_rotate_glwe<9,4,2,3>',
        1520: 'k_blind_rotate_glwe<9,4,2,3>', 1536: 'k_blind_rotate_glwe<9,4,2,3>',
        1537: 'k_blind_rotate_glwe<9,4,2,3>*1536 + k_blind_rotate_glwe<9,4,2,1>*1',
        1919: 'k_blind_rotate_glwe<9,4,2,3>*1536 + k_blind_rotate_glwe<9,4,2,2>*383',
        1920: 'k_blind_rotate_glwe<9,4,2,3>*1536 + k_blind_rotate_glwe<9,4,2,2>*384', 2108: 'k_blind_rotate_glwe<9,4,2,3>',
    }),
    ('k=3 N512 br_glwe_fpw=1', '670 9 3 1 18 6 2 7 2', 'br_glwe_fpw=1', 'br', {
        1: 'k_blind_rotate_glwe<9,4,2,1>', 256: 'k_blind_rotate_glwe<9,4,2,1>', 257: 'k_blind_rotate_glwe<9,4,2,1>',
        512: 'k_blind_rotate_glwe<9,4,2,1>', 513: 'k_blind_rotate_glwe<9,4,2,1>', 768: 'k_blind_rotate_glwe<9,4,2,1>',
        769: 'k_blind_rotate_glwe<9,4,2,1>', 868: 'k_blind_rotate_glwe<9,4,2,1>', 1024: 'k_blind_rotate_glwe<9,4,2,1>',
        1025: 'k_blind_rotate_glwe<9,4,2,1>', 1280: 'k_blind_rotate_glwe<9,4,2,1>', 1281: 'k_blind_rotate_glwe<9,4,2,1>',
        1520: 'k_blind_rotate_glwe<9,4,2,1>', 1536: 'k_blind_rotate_glwe<9,4,2,1>', 1537: 'k_blind_rotate_glwe<9,4,2,1>',
        1919: 'k_blind_rotate_glwe<9,4,2,1>', 1920: 'k_blind_rotate_glwe<9,4,2,1>', 2108: 'k_blind_rotate_glwe<9,4,2,1>',
    }),
    ('k=3 N512 br_glwe_fpw=2', '670 9 3 1 18 6 2 7 2', 'br_glwe_fpw=2', 'br', {
        1: 'k_blind_rotate_glwe<9,4,2,2>', 256: 'k_blind_rotate_glwe<9,4,2,2>', 257: 'k_blind_rotate_glwe<9,4,2,2>',
        512: 'k_blind_rotate_glwe<9,4,2,2>', 513: 'k_blind_rotate_glwe<9,4,2,2>', 768: 'k_blind_rotate_glwe<9,4,2,2>',
        769: 'k_blind_rotate_glwe<9,4,2,2>', 868: 'k_blind_rotate_glwe<9,4,2,2>', 1024: 'k_blind_rotate_glwe<9,4,2,2>',
        1025: 'k_blind_rotate_glwe<9,4,2,2>', 1280: 'k_blind_rotate_glwe<9,4,2,2>', 1281: 'k_blind_rotate_glwe<9,4,2,2>',
        1520: 'k_blind_rotate_glwe<9,4,2,2>', 1536: 'k_blind_rotate_glwe<9,4,2,2>', 1537: 'k_blind_rotate_glwe<9,4,2,2>',
        1919: 'k_blind_rotate_glwe<9,4,2,2>', 1920: 'k_blind_rotate_glwe<9,4,2,2>', 2108: 'k_blind_rotate_glwe<9,4,2,2>',
    }),
    ('k=2 N512', '8 9 2 2 8 4 4 7 1', '', 'br', {
        1: 'k_blind_rotate_glwe<9,3,1,1>', 256: 'k_blind_rotate_glwe<9,3,1,1>', 257: 'k_blind_rotate_glwe<9,3,1,2>',
        512: 'k_blind_rotate_glwe<9,3,1,2>', 513: 'k_blind_rotate_glwe<9,3,1,4>', 768: 'k_blind_rotate_glwe<9,3,1,4>',
        769: 'k_blind_rotate_glwe<9,3,1,4>', 1024: 'k_blind_rotate_glwe<9,3,1,4>',
        1124: 'k_blind_rotate_glwe<9,3,1,4>*1024 + k_blind_rotate_glwe<9,3,1,1>*100',
        1280: 'k_blind_rotate_glwe<9,3,1,4>*1024 + k_blind_rotate_glwe<9,3,1,1>*256',
        1281: 'k_blind_rotate_glwe<9,3,1,4>*1024 + k_blind_rotate_glwe<9,3,1,2>*257',
        1536: 'k_blind_rotate_glwe<9,3,1,4>*1024 + k_blind_rotate_glwe<9,3,1,2>*512', 1537: 'k_blind_rotate_glwe<9,3,1,4>',
        1792: 'k_blind_rotate_glwe<9,3,1,4>', 1793: 'k_blind_rotate_glwe<9,3,1,4>', 1919: 'k_blind_rotate_glwe<9,3,1,4>',
        1920: 'k_blind_rotate_glwe<9,3,1,4>', 2032: 'k_blind_rotate_glwe<9,3,1,4>',
        2108: 'k_blind_rotate_glwe<9,3,1,4>*2048 + k_blind_rotate_glwe<9,3,1,1>*60',
    }),
    ('k=3 N1024', '8 10 3 2 8 4 4 7 1', '', 'br', {
        1: 'k_blind_rotate_glwe<10,4,1,1>', 256: 'k_blind_rotate_glwe<10,4,1,1>', 257: 'k_blind_rotate_glwe<10,4,1,2>',
        512: 'k_blind_rotate_glwe<10,4,1,2>', 513: 'k_blind_rotate_glwe<10,4,1,2>*512 + k_blind_rotate_glwe<10,4,1,1>*1',
        612: 'k_blind_rotate_glwe<10,4,1,2>*512 + k_blind_rotate_glwe<10,4,1,1>*100',
        768: 'k_blind_rotate_glwe<10,4,1,2>*512 + k_blind_rotate_glwe<10,4,1,1>*256', 769: 'k_blind_rotate_glwe<10,4,1,2>',
        1008: 'k_blind_rotate_glwe<10,4,1,2>', 1024: 'k_blind_rotate_glwe<10,4,1,2>',
        1025: 'k_blind_rotate_glwe<10,4,1,2>*1024 + k_blind_rotate_glwe<10,4,1,1>*1',
        1280: 'k_blind_rotate_glwe<10,4,1,2>*1024 + k_blind_rotate_glwe<10,4,1,1>*256',
        1281: 'k_blind_rotate_glwe<10,4,1,2>', 1919: 'k_blind_rotate_glwe<10,4,1,2>', 1920: 'k_blind_rotate_glwe<10,4,1,2>',
        2108: 'k_blind_rotate_glwe<10,4,1,2>*2048 + k_blind_rotate_glwe<10,4,1,1>*60',
    }),
    ('P1024 ks', '630 10 1 3 7 8 2 7 1', '', 'ks', {
        1: 'k_ks_gemm<2,2> (int8 MFMA)', 31: 'k_ks_gemm<2,2> (int8 MFMA)', 32: 'k_ks_gemm<2,2> (int8 MFMA)',
        64: 'k_ks_gemm<2,2> (int8 MFMA)', 65: 'k_ks_gemm<2,2> (int8 MFMA)', 256: 'k_ks_gemm<2,2> (int8 MFMA)',
        2108: 'k_ks_gemm<2,2> (int8 MFMA)',
    }),
    ('P1024 ks_mfma=0', '630 10 1 3 7 8 2 7 1', 'ks_mfma=0', 'ks', {
        1: 'k_keyswitch<8>', 31: 'k_keyswitch<8>', 32: 'k_keyswitch_lanes<8,1,4>', 64: 'k_keyswitch_lanes<8,1,4>',
        65: 'k_keyswitch_fp<8,2,8>', 256: 'k_keyswitch_fp<8,2,8>', 2108: 'k_keyswitch_fp<8,2,8>',
    }),
    ('P1024 ks_mfma=0 ks_fp=0', '630 10 1 3 7 8 2 7 1', 'ks_mfma=0 ks_fp=0', 'ks', {
        1: 'k_keyswitch<8>', 31: 'k_keyswitch<8>', 32: 'k_keyswitch_lanes<8,1,4>', 64: 'k_keyswitch_lanes<8,1,4>',
        65: 'k_keyswitch_lanes<8,2,8>', 256: 'k_keyswitch_lanes<8,2,8>', 2108: 'k_keyswitch_lanes<8,2,8>',
    }),
    # 9-bit key-switch digits do not fit the GEMM's int8 operand (ks_gemm_exact), whatever the int32 sums allow; FP64 has no room either
    ('gamma=9 ks', '12 8 1 2 10 1 9 7 1', '', 'ks', {
        1: 'k_keyswitch<8>', 31: 'k_keyswitch<8>', 32: 'k_keyswitch_lanes<8,1,4>', 64: 'k_keyswitch_lanes<8,1,4>',
        65: 'k_keyswitch_lanes<8,2,8>', 256: 'k_keyswitch_lanes<8,2,8>',
    }),
    ('gamma=8 ks', '12 8 1 2 10 1 8 7 1', '', 'ks', {
        1: 'k_ks_gemm<2,2> (int8 MFMA)', 31: 'k_ks_gemm<2,2> (int8 MFMA)', 32: 'k_ks_gemm<2,2> (int8 MFMA)',
        64: 'k_ks_gemm<2,2> (int8 MFMA)', 65: 'k_ks_gemm<2,2> (int8 MFMA)', 256: 'k_ks_gemm<2,2> (int8 MFMA)',
    }),
]


def select(host, lines):
    """-> one list of (kind, name, first, count) per input line; ("error", code) for a refused parameter set"""
    r = subprocess.run([host, "select"], input="\n".join(lines) + "\n", capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-500:] + r.stderr[-3000:]
    cases = r.stdout.split("\n\n")[:-1]
    assert len(cases) == len(lines)
    out = []
    for block in cases:
        rows = [ln.split("\t") for ln in block.splitlines()]
        out.append([("error", int(x[1])) if x[0] == "error" else (x[0], x[1], int(x[2]), int(x[3])) for x in rows])
    return out


def line(prm, count, knobs=""):
    """harness input: n log_n k l beta t gamma p group cu_count count [knob=value ...]"""
    return f"{prm} {CUS} {count} {knobs}".strip()


def test_every_catalog_entry_is_what_the_selection_picks_for_its_recipe(harness):  # noqa: F811
    from tfhe_fbs_map_amd import _native
    names = _native.kernel_catalog()
    assert len(set(names)) == len(names) >= 160
    lines = []
    for name in names:
        rec = recipe(name)
        assert rec is not None, name
        L = rec["log_n"]        # (the parameter set tests/test_gpu_dispatch.py:run_case makes of a recipe)
        prm = f"{8 if L < 12 else 4} {L} {rec.get('k', 1)} {rec['l']} {rec['beta']} 4 {4 if L < 12 else 3} 7 {rec['group']}"
        lines.append(line(prm, rec["count"], " ".join(f"{k}={v}" for k, v in rec["knobs"].items())))
    for name, launches in zip(names, select(harness[0], lines)):
        assert name in [x[1] for x in launches], (name, launches)


def test_launches_at_the_boundaries_of_every_family(harness):  # noqa: F811
    lines, want = [], []
    for label, prm, knobs, kind, table in BOUNDARIES:
        for count, launches in table.items():
            lines.append(line(prm, count, knobs))
            want.append((label, count, kind, launches))
    for (label, count, kind, launches), got in zip(want, select(harness[0], lines)):
        seq = [x for x in got if x[0] == kind]
        first = 0
        for x in seq:                                  # in order, contiguous, all of the call
            assert x[2] == first and x[3] > 0, (label, count, got)
            first += x[3]
        assert first == count, (label, count, got)
        text = seq[0][1] if len(seq) == 1 else " + ".join(f"{x[1]}*{x[3]}" for x in seq)
        assert text == launches, (label, count, text)


def test_admission_refuses_what_the_context_refuses(harness):  # noqa: F811
    from tfhe_fbs_map_amd import Params
    bad = (Params(k=2, log_n_poly=11), Params(k=5, log_n_poly=9), Params(log_n_poly=13), Params(l_bsk=5, beta_bsk=7), Params(p_msg=0))
    fields = ("n", "log_n_poly", "k", "l_bsk", "beta_bsk", "t_ksk", "gamma_ksk", "p_msg", "bsk_group")
    lines = [line(" ".join(str(getattr(p, f)) for f in fields), 1) for p in bad]   # (test_capi_symbols.py: code -1 from fbs_ctx_create)
    # gadget bases far out of range: refused before q / 2^(beta (lv + 1)) or q / 2^(gamma (v + 1)) is computed
    lines += ["630 10 1 3 200 8 2 7 1 256 1", "630 10 1 3 7 8 200 7 1 256 1", "630 10 1 16 200 64 200 7 1 256 1"]
    assert select(harness[0], lines) == [[("error", -1)]] * len(lines)
    good = select(harness[0], [line("630 10 1 3 7 8 2 7 1", 1)])[0]
    assert good and good[0][0] == "ks"


def test_the_glwe_shapes_of_the_catalog_are_the_ones_params_admits():
    from tfhe_fbs_map_amd import _native
    from tfhe_fbs_map_amd.params import glwe_shape_built
    built = {(int(m.group(1)), int(m.group(2)) - 1) for m in map(re.compile(r"k_blind_rotate_glwe<(\d+),(\d+),\d+,\d+>").fullmatch,
                                                                  _native.kernel_catalog()) if m}
    admitted = {(log_n, k) for log_n in range(2, 15) for k in range(2, 9) if glwe_shape_built(log_n, k)}
    assert built == admitted and len(built) == 8
