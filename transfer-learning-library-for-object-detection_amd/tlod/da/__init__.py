"""Domain-adaptation methods on the detector: DAF (lib/DAF), MAF (lib/MAF), ATF (lib/ATF),
PT-MAF (lib/PT_MAF), US-DAF (lib/US_DAF)."""
