"""`losses.py` of the reference (losses.py:4-16): MSE on coarse (+ fine) rgb.

On the GPU the loss, the PSNR and the backward seed are one HIP launch (`nerfhip_mse_psnr`)
instead of ~14 tiny ATen launches; `MSELoss` keeps the reference's interface and value."""
from torch import nn

from . import ops


class MSELoss(nn.Module):
    def __init__(self):
        super(MSELoss, self).__init__()
        # not used by forward(): it is the attribute the reference's MSELoss has (losses.py:7), so part of the drop-in surface — keep
        self.loss = nn.MSELoss(reduction='mean')
        self.last = None          # [loss, psnr(fine|coarse), mse] of the last forward (detached device tensor)

    def forward(self, inputs, targets):
        loss, self.last = ops.mse_psnr(inputs['rgb_coarse'], inputs.get('rgb_fine'), targets)
        return loss


loss_dict = {'mse': MSELoss}
