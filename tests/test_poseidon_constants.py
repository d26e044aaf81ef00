"""ministark_amd/csrc/poseidon252_constants.h is what scripts/gen_poseidon252_constants.py writes, and its words are the Montgomery
form of the recipe's values: rc[i] = sha256("Hades<i>") mod p, four little-endian u64 of rc[i] 2^256 mod p."""
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ministark_amd", "csrc", "poseidon252_constants.h")
P = (1 << 251) + 17 * (1 << 192) + 1


def test_committed_header_is_what_the_script_generates():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_poseidon252_constants as gen
    assert open(HEADER).read() == gen.render()
    assert gen.OUT == HEADER and gen.P == P


def test_words_are_the_montgomery_form_of_the_recipe():
    text = open(HEADER).read()
    body = text[text.index("RC[91][3][4]"):]
    ws = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", body)]
    assert len(ws) == 273 * 4
    rinv = pow(1 << 256, -1, P)
    for i in range(273):
        m = sum(ws[4 * i + k] << (64 * k) for k in range(4))
        assert m < P, i                                                        # canonical words
        assert m * rinv % P == int(hashlib.sha256(b"Hades%d" % i).hexdigest(), 16) % P, i
    assert ws[0] | ws[1] << 64 | ws[2] << 128 | ws[3] << 192 == (2950795762459345168613727575620414179244544320470208355568817838579231751791 << 256) % P
    two = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", text[text.index("TWO[4]"):text.index("RC[91]")])]
    assert len(two) == 4 and sum(w << (64 * k) for k, w in enumerate(two)) == (2 << 256) % P
    assert "ROUNDS = 91, FULL_HALF = 4" in text
