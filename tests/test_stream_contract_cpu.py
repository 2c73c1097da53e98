"""The table of tests/test_gpu_stream_contract.py against include/sship.h: every function whose parameter list ends in `void* stream` has
a row (ENTRIES) or a stated reason to have none (EXEMPT), so that a new asynchronous entry cannot be added without one."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_entries(text: str):
    """The functions of a C header whose parameter list ends in `void* stream`."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for m in re.finditer(r"\b(sship_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = [a.strip() for a in m.group(2).split(",")]
        if re.fullmatch(r"void\s*\*\s*stream", params[-1]):
            out.append(m.group(1))
    return out


def test_the_parser_finds_what_it_should():
    sample = """int sship_a(int x, void* stream);   /* f(void* stream); in a comment */
    int sship_b(const float* p,
                void *stream);
    int sship_c(void* stream, int n);
    void sship_d(void (*cb)(int level, const char* msg));
    int sship_e(void);"""
    assert stream_entries(sample) == ["sship_a", "sship_b"]


def test_every_entry_that_takes_a_stream_has_a_row_or_a_reason():
    import test_gpu_stream_contract as T
    from superslam_amd import _lib

    with open(os.path.join(ROOT, "include", "sship.h")) as f:
        header = stream_entries(f.read())
    assert len(header) == len(set(header)) and len(header) >= 40, header
    table = set(T.ENTRIES) | set(T.EXEMPT)
    assert not set(T.ENTRIES) & set(T.EXEMPT)
    assert sorted(set(header) - table) == [], "asynchronous entries without a row in tests/test_gpu_stream_contract.py"
    assert sorted(table - set(header)) == [], "rows that name no function of include/sship.h that takes a stream"
    assert sorted(table - set(_lib._SIGS)) == [], "rows that superslam_amd._lib does not bind"
    for name, cases in T.ENTRIES.items():
        assert cases and all(isinstance(cid, str) and callable(fn) for cid, fn in cases), name
    ids = [cid for cid, _ in T.CASES]                      # a case may cover two entries (an add, then the query that reads it); it runs once
    assert len(ids) == len(set(ids))
    for name, reason in T.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 20, name
