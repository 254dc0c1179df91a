"""Shared by tests/test_attention_maps_host.py and tests/test_hip_attention_maps.py: the ChaosAttention construction whose maps are far
from uniform, and the reference's attention weights written out unfolded."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch            # noqa: E402

from smokephysai_amd.models import ChaosAttention            # noqa: E402


def peaked_module(dim=128, heads=2, weight_scale=4.0, seed=0):
    """A ChaosAttention with temperature 0.7, chaos_strength 0.5 and q_proj / k_proj weights scaled up, so that its softmax rows are far from
    uniform (tests/test_hip_attention_maps.py reuses it)."""
    torch.manual_seed(seed)
    m = ChaosAttention(dim, heads, chaos_strength=0.5, temperature=0.7).eval()
    with torch.no_grad():
        m.q_proj.weight.mul_(weight_scale)
        m.k_proj.weight.mul_(weight_scale)
    return m


def module_inputs(B=2, L=128, dim=128, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, dim, generator=g), torch.randn(3, B, 1, generator=g)


def reference_probs(m, x, noise):
    """attn_weights of the reference's forward, written out unfolded: two score tensors, the gate as a row scaling, softmax over
    final_scores / temperature (chaos_attention.py:77-108)."""
    B, L, D = x.shape
    H, d = m.num_heads, m.head_dim
    q = m.q_proj(x).view(B, L, H, d).transpose(1, 2)
    k = m.k_proj(x).view(B, L, H, d).transpose(1, 2)
    scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(d)
    chaos_features = m.chaos_proj(m.generate_chaos_field(L, B, x.device, noise).to(x.dtype))
    gate = torch.sigmoid(m.chaos_gate(chaos_features)).unsqueeze(1)
    chaos_scores = torch.matmul(chaos_features.view(B, L, H, d).transpose(1, 2), k.transpose(-2, -1)) / math.sqrt(d)
    final = scores + m.chaos_strength * chaos_scores * gate
    return torch.softmax(final / m.temperature, dim=-1)
