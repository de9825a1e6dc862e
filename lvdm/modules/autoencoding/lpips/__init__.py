"""Drop-in import path of the reference (`lvdm...`): only the modules of the encode/decode path, its frozen 2-D constraint decoder and the LPIPS perceptual loss exist here."""
