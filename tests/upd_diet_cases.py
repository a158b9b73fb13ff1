"""Cases of tests/test_upd_counts_emulated.py and tests/test_upd_counts_gpu.py: the smallest shapes that reach every branch of k_iter_update's
partner pass since it counts the digit pairs of a partner row ONCE, under the key they gain with the new row, and reads what A's and B's blocks
lose through the inverse map (upd_loss, cmvm_engine.hip).  Every case is one wmc chain (the greedy loop alone) compared with the oracle, whole Pipeline.

group -> [int_matrix arguments]
  same_row   12x10 and 16x16 int8: picks of a row with itself (A == B: both loss vectors land in A's block), adding and subtracting picks, partner rows
             below and above A and B (mirrored keys and plain ones).  The tests check on the oracle's op lists that these picks occur.
  shifts     8x8 with entries up to +-127: eight digits, shifts of up to seven positions push B's key index to both ends of the count vector
  long_rows  6x40, 4x64, 3x96 int8: partner rows of more than 32 and more than 64 list entries (both settings of DA_UPD_CH and the tail loop)
  wide_cells 8x8 with 15-bit entries and 2x300: 64-bit cells, 16-byte list entries, count vectors of up to 58 keys
  passes     48x16 int8: more partner rows than one pass of two update blocks takes (run with DA4ML_HIP_UPD_BLOCKS=2), and -- with a small
             DA4ML_HIP_TABLE_SCALE -- blocks beyond their home bucket and creations into a full bucket"""

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)

GROUPS = {
    'same_row': [(0, 12, 10, -128, 128), (1, 12, 10, -128, 128), (0, 16, 16, -128, 128), (3, 16, 16, -128, 128)],
    'shifts': [(0, 8, 8, -127, 128), (1, 8, 8, -127, 128), (2, 8, 8, -127, 128)],
    'long_rows': [(0, 6, 40, -128, 128), (0, 4, 64, -128, 128), (0, 3, 96, -128, 128)],
    'wide_cells': [(0, 8, 8, -(2**14), 2**14), (0, 2, 300, -8, 8)],
    'passes': [(0, 48, 16, -128, 128)],
}

# DA4ML_HIP_TABLE_SCALE of the `passes` chain: the tightest table at which the chain still completes without the capacity retry.  Scanned on the
# emulated device with DA4ML_HIP_UPD_BLOCKS=2: 1 and 0.5 complete at once, 0.4, 0.3, 0.2 and 0.15 retry once, 0.1, 0.07 and 0.05 twice.
TIGHT_TABLE_SCALE = '0.5'


def self_pairs(p):
    """(adding, subtracting) picks of a row with itself in a Pipeline: operations on two copies of one value"""
    add = sub = 0
    for s in p.solutions:
        for op in s.ops:
            if op.opcode in (0, 1) and op.id0 == op.id1 and op.id0 >= 0:
                add += op.opcode == 0
                sub += op.opcode == 1
    return add, sub
