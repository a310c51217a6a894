"""The oracle's carried mode of comprox / comprolz against the unmodified reference library run block after block behind ONE
reset_models(). Only hand-made cases whose blocks are all coded: the reference trusts its input behind tiny and stored blocks."""
import pytest

import crlib


@pytest.mark.parametrize("name", ["text3", "repeat", "families"])
@pytest.mark.parametrize("which", ["rox", "rolz"])
def test_carried_sequences_match_the_reference(oracle, which, name):
    if not crlib.Reference.available(which):
        pytest.skip("oracle/_ref not built (no /root/reference)")
    enc, dec = (oracle.rox_encode, oracle.rox_decode) if which == "rox" else (oracle.rolz_encode, oracle.rolz_decode)
    blocks, ref = [bytes(b) for b in dict(crlib.CASES)[name]], crlib.Reference(which)
    coded = [enc(b, reset=(i == 0)) for i, b in enumerate(blocks)]
    assert ref.encode_sequence(blocks) == coded and ref.decode_sequence(coded) == blocks
    assert [dec(e, len(b), reset=(i == 0)) for i, (e, b) in enumerate(zip(coded, blocks))] == blocks
