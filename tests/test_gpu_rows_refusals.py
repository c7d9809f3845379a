"""The return codes of the fused scorer's four calls for requests they refuse (and for the empty requests they accept), through ctypes:
drx_rows_recommend / drx_rows_rank_items / drx_rows_rank_lists / drx_rows_pair_scores.  The ORDER of the refusals is part of the
behaviour (a request wrong in two ways has one answer), so every case asserts the exact code.  EXPECTED was recorded from the library
before the four calls got one shared request check; a case a call has no argument for is absent from its column.

Tensors of a few rows: n_items = 40, ld = 8, R = 3 (allocated 260 floats a row, so that a call at ld = 260 reads inside them).
"""
import pytest

pytestmark = pytest.mark.gpu

OK, EINVAL, ESCRATCH, ENOTIMPL = 0, -1, -2, -3
SIGMOID_BIAS, BIAS, CLIP = 0, 1, 2
N, LD, R, WIDE = 40, 8, 3, 260
CALLS = ('recommend', 'rank_items', 'rank_lists', 'pair_scores')

# case -> what it changes of a valid BIAS request.  'scratch': None = a null pointer, an int = that many bytes short of what the
# call's size function asks for, 'tiny' = 64 bytes
CASES = {
    'valid': {},
    'null table': {'table': None},
    'null q': {'q': None},
    'null first output': {'out0': None},
    'null second output': {'out1': None},
    'null targets': {'targets': None},
    'null target offsets': {'tptr': None},
    'ld 0': {'ld': 0},
    'ld 2': {'ld': 2},
    'ld 6': {'ld': 6},
    'epilogue 3': {'epilogue': 3},
    'clip with a bias': {'epilogue': CLIP},
    'sigmoid without a bias': {'epilogue': SIGMOID_BIAS, 'bias': None},
    'exclusion offsets alone': {'xptr': True},
    'exclusion items alone': {'xidx': True},
    'exclusions without uid': {'xptr': True, 'xidx': True, 'uid': None},
    'n 129': {'n': 129},
    'n 129, null scratch': {'n': 129, 'scratch': None},
    'ld 260': {'ld': WIDE},
    'ld 260, null scratch': {'ld': WIDE, 'scratch': None},
    'null scratch': {'scratch': None},
    'scratch one byte short': {'scratch': 1},
    'scratch of 64 bytes': {'scratch': 'tiny'},
    'no targets, null scratch': {'no_targets': True, 'scratch': None},
    'P 0, null pointers': {'P': 0, 'table': None, 'q': None, 'out0': None, 'rows': None},
    'P 0, epilogue 3': {'P': 0, 'epilogue': 3},
    'ld 260, n 129': {'ld': WIDE, 'n': 129},                      # (wrong in two ways: the code of the first check that fires)
    'epilogue 3, null scratch': {'epilogue': 3, 'scratch': None},
}
ONLY = {'n 129': ('recommend',), 'n 129, null scratch': ('recommend',), 'ld 260, n 129': ('recommend',),
        'no targets, null scratch': ('rank_lists',), 'P 0, null pointers': ('pair_scores',), 'P 0, epilogue 3': ('pair_scores',),
        'null second output': CALLS[:3], 'null targets': CALLS[1:3], 'null target offsets': ('rank_lists',)}
NOT_FOR_PAIRS = ('exclusion offsets alone', 'exclusion items alone', 'exclusions without uid', 'null scratch', 'scratch one byte short',
                 'scratch of 64 bytes', 'ld 260, null scratch', 'epilogue 3, null scratch')

# case -> the codes of the calls it applies to, in CALLS' order
CODES = {
    'valid': (OK, OK, OK, OK),
    'null table': (EINVAL, EINVAL, EINVAL, EINVAL),
    'null q': (EINVAL, EINVAL, EINVAL, EINVAL),
    'null first output': (EINVAL, EINVAL, EINVAL, EINVAL),
    'null second output': (EINVAL, EINVAL, EINVAL),
    'null targets': (EINVAL, EINVAL),
    'null target offsets': (EINVAL,),
    'ld 0': (EINVAL, EINVAL, EINVAL, EINVAL),
    'ld 2': (EINVAL, EINVAL, EINVAL, EINVAL),
    'ld 6': (EINVAL, EINVAL, EINVAL, EINVAL),
    'epilogue 3': (EINVAL, EINVAL, EINVAL, EINVAL),
    'clip with a bias': (EINVAL, EINVAL, EINVAL, EINVAL),
    'sigmoid without a bias': (EINVAL, EINVAL, EINVAL, EINVAL),
    'exclusion offsets alone': (EINVAL, EINVAL, EINVAL),
    'exclusion items alone': (EINVAL, EINVAL, EINVAL),
    'exclusions without uid': (EINVAL, EINVAL, EINVAL),
    'n 129': (ENOTIMPL,),
    'n 129, null scratch': (ENOTIMPL,),
    'ld 260': (ENOTIMPL, ENOTIMPL, ENOTIMPL, OK),
    'ld 260, null scratch': (ENOTIMPL, ENOTIMPL, ENOTIMPL),
    'null scratch': (ESCRATCH, ESCRATCH, ESCRATCH),
    'scratch one byte short': (OK, OK, ESCRATCH),     # (the first two carve inside the size function's 256 bytes of slack; rank_lists
                                                      #  holds the caller to the size function's answer to the byte)
    'scratch of 64 bytes': (ESCRATCH, ESCRATCH, ESCRATCH),
    'no targets, null scratch': (OK,),
    'P 0, null pointers': (OK,),
    'P 0, epilogue 3': (EINVAL,),
    'ld 260, n 129': (ENOTIMPL,),
    'epilogue 3, null scratch': (EINVAL, EINVAL, EINVAL),
}


def applies(case, call):
    return call in ONLY.get(case, CALLS) and not (call == 'pair_scores' and case in NOT_FOR_PAIRS)


EXPECTED = {(call, case): code for case, codes in CODES.items() for call, code in zip([c for c in CALLS if applies(case, c)], codes)}


class Request:
    """one valid request of every call on shared tensors; code(call, case) = the return code with the case's changes applied"""

    def __init__(self):
        import torch
        self.torch = torch
        dev = torch.device('cuda:0')
        g = torch.Generator(device='cpu').manual_seed(3)
        self.table = torch.randn(N * WIDE, generator=g).to(dev)
        self.q = torch.randn(R * WIDE, generator=g).to(dev)
        self.bias = torch.randn(N, generator=g).to(dev)
        self.uid = torch.arange(R, dtype=torch.int32, device=dev)
        self.rows = torch.arange(R, dtype=torch.int32, device=dev)                    # targets of the rank calls, q_row / t_row of pair_scores
        self.tptr = torch.arange(R + 1, dtype=torch.int64, device=dev)                # one target per row
        self.no_tptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        self.xptr = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device=dev)
        self.xidx = torch.tensor([5, 6, 7], dtype=torch.int32, device=dev)
        self.out_i = torch.empty(R * 129, dtype=torch.int32, device=dev)
        self.out_f = torch.empty(R * 129, dtype=torch.float32, device=dev)
        self.scratch = torch.empty(8 << 20, dtype=torch.uint8, device=dev)

    def code(self, call, case):
        from drecpy_amd import _lib
        L, c = _lib.lib(), CASES[case]
        arg = lambda key, tensor: _lib.ptr(c.get(key, tensor))                       # (a case names a tensor only to pass NULL for it)
        ld, n, epilogue = c.get('ld', LD), c.get('n', 4), c.get('epilogue', BIAS)
        table, q, bias = arg('table', self.table), arg('q', self.q), arg('bias', self.bias)
        st = _lib.stream_ptr(self.torch.device('cuda:0'))
        if call == 'pair_scores':
            rows = arg('rows', self.rows)
            rc = L.drx_rows_pair_scores(table, bias, N, ld, epilogue, q, R, rows, rows, c.get('P', R), arg('out0', self.out_f), st)
        else:
            need = int({'recommend': lambda: L.drx_rows_recommend_scratch_bytes(R, N, LD, 4),
                        'rank_items': lambda: L.drx_rows_rank_items_scratch_bytes(R, N, LD),
                        'rank_lists': lambda: L.drx_rows_rank_lists_scratch_bytes(R, R, N, LD)}[call]())
            assert 0 < need <= self.scratch.numel()
            short = c.get('scratch', 0)
            scratch = _lib.ptr(None if short is None else self.scratch)
            nbytes = 0 if short is None else 64 if short == 'tiny' else need - short
            uid = arg('uid', self.uid)
            xptr, xidx = _lib.ptr(self.xptr if c.get('xptr') else None), _lib.ptr(self.xidx if c.get('xidx') else None)
            o0, o1 = arg('out0', self.out_i), arg('out1', self.out_f)
            if call == 'recommend':
                rc = L.drx_rows_recommend(table, bias, N, ld, epilogue, q, uid, R, n, xptr, xidx, o0, o1, scratch, nbytes, st)
            elif call == 'rank_items':
                rc = L.drx_rows_rank_items(table, bias, N, ld, epilogue, q, uid, arg('targets', self.rows), R, xptr, xidx, o0, o1, scratch, nbytes, st)
            else:
                tptr = arg('tptr', self.no_tptr if c.get('no_targets') else self.tptr)
                rc = L.drx_rows_rank_lists(table, bias, N, ld, epilogue, q, uid, R, tptr, arg('targets', self.rows), xptr, xidx, o0, o1, scratch,
                                           nbytes, st)
        self.torch.cuda.synchronize()
        return int(rc)


@pytest.fixture(scope='module')
def rq():
    return Request()


def test_the_table_covers_every_case_of_every_call():
    assert list(CODES) == list(CASES)
    assert all(len(codes) == sum(applies(case, call) for call in CALLS) for case, codes in CODES.items())


@pytest.mark.parametrize('call,case', sorted(EXPECTED))
def test_refusal_code(rq, call, case):
    assert rq.code(call, case) == EXPECTED[call, case]
