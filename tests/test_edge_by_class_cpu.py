"""The host side of the pair tensor by class (ops.PairByClass, EmbeddingModule.et_by_class = S2S_ET_BY_CLASS): the buffer's offsets, the
switch and its place in the sampler's graph key."""
import pytest
import torch

from str2str_amd import ops


@pytest.mark.parametrize("B,N", [(1, 1), (3, 7), (2, 33), (2, 37), (128, 256)])
@pytest.mark.parametrize("rec", [128, 168])
def test_buffer_offsets(B, N, rec):
    """[M32 index words | zero record | class records]: M32 = B N^2 rounded up to 32, so the records start 16-byte aligned (128 B, in fact)."""
    M = B * N * N
    M32 = ops.PairByClass.index_words(B, N)
    assert M <= M32 < M + 32 and M32 % 32 == 0 and (M32 * 4) % 16 == 0 and (rec * 4) % 16 == 0
    rows = 5
    buf = torch.arange(M32 + (rows + 1) * rec, dtype=torch.float32)
    p = ops.PairByClass(B, N, buf, rec)
    assert (p.M32, p.rec, p.shape, p.data_ptr()) == (M32, rec, (B, N, N, 128), buf.data_ptr()) and p.contiguous() is p
    assert p.index.shape == (B, N, N) and p.index.dtype == torch.int32 and p.index.data_ptr() == buf.data_ptr()
    assert p.records.shape == (rows + 1, rec) and p.records.data_ptr() == buf.data_ptr() + 4 * M32
    assert p.records[1, 0].item() == M32 + rec            # class r = record r + 1: the zero record comes first
    with pytest.raises(ops.HipLibraryError):
        ops.PairByClass(B, N, buf[:-1], rec)              # not a whole number of records
    with pytest.raises(ops.HipLibraryError):
        ops.PairByClass(B, N, buf, 160)
    with pytest.raises(ops.HipLibraryError):
        ops.pair_untiled(p)                               # no producer: nothing to expand with


def test_switch_values_and_graph_key(monkeypatch):
    from str2str_amd.factory import build_synthetic_net
    from str2str_amd.models.net.denoising_ipa import EmbeddingModule
    from str2str_amd.sampler import _graph_key

    assert EmbeddingModule.launch_modes == ("ee_classes", "et_by_class") and "et_by_class" not in EmbeddingModule.launch_switches
    net = build_synthetic_net(seed=0, sigma_final=0.02, device="cpu")
    assert net.embedder.et_by_class == "auto"
    for value in ("auto", "0", "1"):
        monkeypatch.setenv("S2S_ET_BY_CLASS", value)
        assert build_synthetic_net(seed=0, sigma_final=0.02, device="cpu").embedder.et_by_class == value
    monkeypatch.setenv("S2S_ET_BY_CLASS", "yes")
    with pytest.raises(ValueError, match="S2S_ET_BY_CLASS"):
        build_synthetic_net(seed=0, sigma_final=0.02, device="cpu")
    # a captured graph holds the launches of one switch value: the key tells them apart
    feats = {"residue_idx": torch.arange(5)[None], "fixed_mask": torch.zeros(1, 5)}
    keys = []
    for value in ("auto", "0", "1", "auto"):
        net.embedder.et_by_class = value
        keys.append(_graph_key(net, feats, 1, 5))
    assert keys[0] == keys[3] and len(set(keys)) == 3
