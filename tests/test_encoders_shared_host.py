"""The encoders' one ``from_pretrained`` (reptext_amd.encoder_common) on directories written by `transformers`' own ``save_pretrained``
(CPU, no kernels involved). transformers 5.x records the model's ``dtype`` in ``config.json``; the text encoders used to pass it on to
their constructor beside their own ``dtype=`` and fail with "got multiple values for keyword argument 'dtype'"."""
import json
import os

import torch


def _check_loads(hf, cls, tmp_path, rename=lambda k: k):
    hf.save_pretrained(str(tmp_path), safe_serialization=True)
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        assert "dtype" in json.load(f)                       # what the loader has to drop: without it this test would show nothing
    mine = cls.from_pretrained(str(tmp_path))
    assert mine.dtype == torch.bfloat16 and mine.device.type == "cpu"
    want = {rename(k): v.to(torch.bfloat16) for k, v in hf.state_dict().items() if k != "encoder.embed_tokens.weight" and not k.endswith("position_ids")}
    got = mine.state_dict()
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v), k


def test_t5_encoder_loads_a_directory_saved_by_transformers(tmp_path):
    from transformers import T5Config
    from transformers import T5EncoderModel as HFT5
    from reptext_amd.text_encoders import T5EncoderModel

    torch.manual_seed(0)
    cfg = T5Config(vocab_size=64, d_model=128, d_kv=64, d_ff=192, num_layers=1, num_heads=2, feed_forward_proj="gated-gelu", is_encoder_decoder=False)
    _check_loads(HFT5(cfg).eval(), T5EncoderModel, tmp_path)


def test_clip_text_model_loads_a_directory_saved_by_transformers(tmp_path):
    from transformers import CLIPTextConfig
    from transformers import CLIPTextModel as HFCLIP
    from reptext_amd.text_encoders import CLIPTextModel

    torch.manual_seed(1)
    cfg = CLIPTextConfig(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, max_position_embeddings=16)
    # transformers >= 5 saves the keys without the `text_model.` prefix, earlier versions with it
    _check_loads(HFCLIP(cfg).eval(), CLIPTextModel, tmp_path, rename=lambda k: k if k.startswith("text_model.") else "text_model." + k)
