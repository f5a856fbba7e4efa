// sbl_dna.h -- DNASequence::Translate (reference src/dnasequence.cpp:11-28) for one byte, shared by the kernels that spell a reverse strand
// from the original records (spell_text.hip, boundary_align.hip): A <-> T and C <-> G in either case, every other byte unchanged.
#pragma once

__device__ inline unsigned char complement1(unsigned char c)
{
	const unsigned char f = c & 0xDF;
	return f == 'A' || f == 'T' ? c ^ 0x15 : f == 'C' || f == 'G' ? c ^ 0x04 : c;
}
