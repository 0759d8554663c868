"""The host twin of the Markov-chain walker (c3control_simulate_chain, libc3sc.so) against the numpy restatement
tests/chain_ref.py, no GPU: 64 walks of 24 steps on the lqg2d case over the user's callbacks, replayed in lock-step."""
import chain_facade_child as child


def test_host_twin_against_the_numpy_reference(oracle):
    out = child.host_twin_against_reference()
    assert out["steps"] == 64 * 24 and out["unsure"] <= 0.025 * out["steps"]
