"""MI355X-native DeepLabv2/ResNet-101 MaxSquare domain-adaptation training step.

Mirrors the reference's layout for the hot path only:
  graphs/models/deeplab_multi.py  - DeeplabMulti with HIP dilated convs / ASPP / upsample
  utils/loss.py                   - MaxSquareloss, IW_MaxSquareloss, softCrossEntropy, IWsoftCrossEntropy, CrossEntropyLoss (fused HIP)
  utils/optim.py                  - SGD and Adam (--optim) with the reference's duplicated-parameter
                                    semantics, each a fused HIP step over every parameter
  utils/dist.py                   - bucketed RCCL all-reduce overlapped with the backward
  tools/solve_gta5.py, tools/train_source.py - the trainer entry points
Native code: csrc/*.hip -> _lib/libmsl_hip.so (C-ABI in include/msl_hip.h).
"""
__version__ = "0.1.0"

import torch as _torch

# The reference computes in fp32 (PyTorch-CPU / cuDNN fp32).  On ROCm, PyTorch's default
# allow_tf32=True lets MIOpen/hipBLASLt run "fp32" convolutions and GEMMs at reduced
# precision, which moves layer1 outputs by ~0.5% and the logits by ~50% after 100 layers
# with bs=1 batch-norm.  The MI355X path keeps every op in true fp32.
_torch.backends.cudnn.allow_tf32 = False
_torch.backends.cuda.matmul.allow_tf32 = False
