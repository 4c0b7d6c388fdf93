// text_common.hpp -- the number core and the block layout of the device text formatter
// (lpr_text_*): the bytes of TableIterationFormater.Format
// (Utilities/TableIterationFormater.cs:22-48) without its title line.  Shared by the kernels
// (text_kernels.hip), the host (text_engine.hip) and a plain host compiler
// (tools/text_format_check.cpp): no HIP header, no floating-point operation, no builtin beyond
// __int128 and __builtin_clzll-class integer code.
//
// The number rule, {v:F3} on .NET Framework (table_iteration_formater.format_fixed):
//   1. NaN prints NaN, the infinities Infinity / -Infinity.
//   2. |v| is first turned into its 15-significant-digit decimal image, correctly rounded, exact
//      ties to even (what "%.14e" gives).
//   3. That image is rounded half AWAY from zero at three decimals.
//   4. Fixed-point, no sign when every printed digit is zero.
//   5. |v| >= 1e15 prints the 15 (after a carry 16) digits, then zeros, then ".000".
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define LPR_TEXT_HD __host__ __device__ inline
#else
#define LPR_TEXT_HD inline
#endif

namespace lpr {

constexpr int kTextDecimals = 3;  // F3; the scaled value T below counts thousandths
// The smallest double that prints 0.001: its 15-digit image is 4.99999999999999(6..)e-4 -> rounds
// to 5.00000000000000e-4 -> half away -> 0.001.  Its predecessor's image is 4.99999999999999e-4.
// tests/test_text_format_cpu.py recomputes it from format_fixed by bisection.
constexpr uint64_t kTextF3Threshold = 0x3F40624DD2F1A9F8ull;
constexpr uint64_t kTextAbsMask = ~(1ull << 63);
constexpr uint64_t kTextInfBits = 0x7FF0000000000000ull;
constexpr uint64_t kTextBigBits = 0x430C6BF526340000ull;  // 1e15 = 2^15 * 5^15, exact in a double
constexpr int kTextMaxCell = 314;  // "-", the 309 digits of DBL_MAX, ".000"

constexpr uint64_t text_ipow(uint64_t b, int n) {
    uint64_t r = 1;
    for (int i = 0; i < n; ++i) r *= b;
    return r;
}
static_assert(text_ipow(5, 18) == 3814697265625ull, "5^18 < 2^42: m * 5^s stays below 2^95");
static_assert(text_ipow(10, 19) == 10000000000000000000ull, "10^19 < 2^64");

enum TextClass : uint8_t { kTextNaN = 0, kTextPosInf, kTextNegInf, kTextZero, kTextFast, kTextBig };

// The bits of the smallest double >= 10^k, k = -4 .. 308 (index k + 4).  Positive doubles order as
// their bit patterns, so `bits >= table[k + 4]` is `|v| >= 10^k`, exactly.  Generated with
// fractions.Fraction(10) ** k, float() and nextafter; tests/test_text_format_cpu.py regenerates
// every entry and compares.
constexpr int kTextPow10Min = -4, kTextPow10Max = 308;
LPR_TEXT_HD uint64_t text_pow10_ceil(int k) {
    static constexpr uint64_t tab[kTextPow10Max - kTextPow10Min + 1] = {
        0x3F1A36E2EB1C432DULL, 0x3F50624DD2F1A9FCULL, 0x3F847AE147AE147BULL, 0x3FB999999999999AULL,
        0x3FF0000000000000ULL, 0x4024000000000000ULL, 0x4059000000000000ULL, 0x408F400000000000ULL,
        0x40C3880000000000ULL, 0x40F86A0000000000ULL, 0x412E848000000000ULL, 0x416312D000000000ULL,
        0x4197D78400000000ULL, 0x41CDCD6500000000ULL, 0x4202A05F20000000ULL, 0x42374876E8000000ULL,
        0x426D1A94A2000000ULL, 0x42A2309CE5400000ULL, 0x42D6BCC41E900000ULL, 0x430C6BF526340000ULL,
        0x4341C37937E08000ULL, 0x4376345785D8A000ULL, 0x43ABC16D674EC800ULL, 0x43E158E460913D00ULL,
        0x4415AF1D78B58C40ULL, 0x444B1AE4D6E2EF50ULL, 0x4480F0CF064DD592ULL, 0x44B52D02C7E14AF7ULL,
        0x44EA784379D99DB5ULL, 0x45208B2A2C280291ULL, 0x4554ADF4B7320335ULL, 0x4589D971E4FE8402ULL,
        0x45C027E72F1F1282ULL, 0x45F431E0FAE6D722ULL, 0x46293E5939A08CEAULL, 0x465F8DEF8808B025ULL,
        0x4693B8B5B5056E17ULL, 0x46C8A6E32246C99DULL, 0x46FED09BEAD87C04ULL, 0x4733426172C74D83ULL,
        0x476812F9CF7920E3ULL, 0x479E17B84357691CULL, 0x47D2CED32A16A1B2ULL, 0x48078287F49C4A1EULL,
        0x483D6329F1C35CA5ULL, 0x48725DFA371A19E7ULL, 0x48A6F578C4E0A061ULL, 0x48DCB2D6F618C879ULL,
        0x4911EFC659CF7D4CULL, 0x49466BB7F0435C9FULL, 0x497C06A5EC5433C7ULL, 0x49B18427B3B4A05CULL,
        0x49E5E531A0A1C873ULL, 0x4A1B5E7E08CA3A90ULL, 0x4A511B0EC57E649AULL, 0x4A8561D276DDFDC1ULL,
        0x4ABABA4714957D31ULL, 0x4AF0B46C6CDD6E3FULL, 0x4B24E1878814C9CEULL, 0x4B5A19E96A19FC41ULL,
        0x4B905031E2503DA9ULL, 0x4BC4643E5AE44D13ULL, 0x4BF97D4DF19D6058ULL, 0x4C2FDCA16E04B86EULL,
        0x4C63E9E4E4C2F345ULL, 0x4C98E45E1DF3B016ULL, 0x4CCF1D75A5709C1BULL, 0x4D03726987666191ULL,
        0x4D384F03E93FF9F5ULL, 0x4D6E62C4E38FF873ULL, 0x4DA2FDBB0E39FB48ULL, 0x4DD7BD29D1C87A1AULL,
        0x4E0DAC74463A98A0ULL, 0x4E428BC8ABE49F64ULL, 0x4E772EBAD6DDC73DULL, 0x4EACFA698C95390CULL,
        0x4EE21C81F7DD43A8ULL, 0x4F16A3A275D49492ULL, 0x4F4C4C8B1349B9B6ULL, 0x4F81AFD6EC0E1412ULL,
        0x4FB61BCCA7119916ULL, 0x4FEBA2BFD0D5FF5CULL, 0x502145B7E285BF99ULL, 0x50559725DB272F80ULL,
        0x508AFCEF51F0FB5FULL, 0x50C0DE1593369D1CULL, 0x50F5159AF8044463ULL, 0x512A5B01B605557BULL,
        0x516078E111C3556DULL, 0x5194971956342AC8ULL, 0x51C9BCDFABC1357AULL, 0x5200160BCB58C16DULL,
        0x52341B8EBE2EF1C8ULL, 0x526922726DBAAE3AULL, 0x529F6B0F092959C8ULL, 0x52D3A2E965B9D81DULL,
        0x53088BA3BF284E24ULL, 0x533EAE8CAEF261ADULL, 0x53732D17ED577D0CULL, 0x53A7F85DE8AD5C4FULL,
        0x53DDF67562D8B363ULL, 0x5412BA095DC7701EULL, 0x5447688BB5394C26ULL, 0x547D42AEA2879F2FULL,
        0x54B249AD2594C37DULL, 0x54E6DC186EF9F45DULL, 0x551C931E8AB87174ULL, 0x5551DBF316B346E8ULL,
        0x558652EFDC6018A2ULL, 0x55BBE7ABD3781ECBULL, 0x55F170CB642B133FULL, 0x5625CCFE3D35D80FULL,
        0x565B403DCC834E12ULL, 0x569108269FD210CCULL, 0x56C54A3047C694FEULL, 0x56FA9CBC59B83A3EULL,
        0x5730A1F5B8132467ULL, 0x5764CA732617ED80ULL, 0x5799FD0FEF9DE8E0ULL, 0x57D03E29F5C2B18CULL,
        0x58044DB473335DEFULL, 0x583961219000356BULL, 0x586FB969F40042C6ULL, 0x58A3D3E2388029BCULL,
        0x58D8C8DAC6A0342BULL, 0x590EFB1178484135ULL, 0x59435CEAEB2D28C1ULL, 0x59783425A5F872F2ULL,
        0x59AE412F0F768FAEULL, 0x59E2E8BD69AA19CDULL, 0x5A17A2ECC414A040ULL, 0x5A4D8BA7F519C850ULL,
        0x5A827748F9301D32ULL, 0x5AB7151B377C247FULL, 0x5AECDA62055B2D9EULL, 0x5B22087D4358FC83ULL,
        0x5B568A9C942F3BA4ULL, 0x5B8C2D43B93B0A8CULL, 0x5BC19C4A53C4E698ULL, 0x5BF6035CE8B6203EULL,
        0x5C2B843422E3A84DULL, 0x5C6132A095CE4930ULL, 0x5C957F48BB41DB7CULL, 0x5CCADF1AEA12525BULL,
        0x5D00CB70D24B7379ULL, 0x5D34FE4D06DE5057ULL, 0x5D6A3DE04895E46DULL, 0x5DA066AC2D5DAEC4ULL,
        0x5DD4805738B51A75ULL, 0x5E09A06D06E26113ULL, 0x5E400444244D7CACULL, 0x5E7405552D60DBD7ULL,
        0x5EA906AA78B912CCULL, 0x5EDF485516E7577FULL, 0x5F138D352E5096B0ULL, 0x5F48708279E4BC5BULL,
        0x5F7E8CA3185DEB72ULL, 0x5FB317E5EF3AB328ULL, 0x5FE7DDDF6B095FF1ULL, 0x601DD55745CBB7EDULL,
        0x6052A5568B9F52F5ULL, 0x60874EAC2E8727B2ULL, 0x60BD22573A28F19EULL, 0x60F2357684599703ULL,
        0x6126C2D4256FFCC3ULL, 0x615C73892ECBFBF4ULL, 0x6191C835BD3F7D79ULL, 0x61C63A432C8F5CD7ULL,
        0x61FBC8D3F7B3340CULL, 0x62315D847AD00088ULL, 0x6265B4E5998400AAULL, 0x629B221EFFE500D4ULL,
        0x62D0F5535FEF2085ULL, 0x630532A837EAE8A6ULL, 0x633A7F5245E5A2CFULL, 0x63708F936BAF85C2ULL,
        0x63A4B378469B6732ULL, 0x63D9E056584240FEULL, 0x64102C35F729689FULL, 0x6444374374F3C2C7ULL,
        0x647945145230B378ULL, 0x64AF965966BCE056ULL, 0x64E3BDF7E0360C36ULL, 0x6518AD75D8438F44ULL,
        0x654ED8D34E547314ULL, 0x6583478410F4C7EDULL, 0x65B819651531F9E8ULL, 0x65EE1FBE5A7E7862ULL,
        0x6622D3D6F88F0B3DULL, 0x665788CCB6B2CE0DULL, 0x668D6AFFE45F8190ULL, 0x66C262DFEEBBB0FAULL,
        0x66F6FB97EA6A9D38ULL, 0x672CBA7DE5054486ULL, 0x6761F48EAF234AD4ULL, 0x679671B25AEC1D89ULL,
        0x67CC0E1EF1A724EBULL, 0x680188D357087713ULL, 0x6835EB082CCA94D8ULL, 0x686B65CA37FD3A0EULL,
        0x68A11F9E62FE4449ULL, 0x68D56785FBBDD55BULL, 0x690AC1677AAD4AB1ULL, 0x6940B8E0ACAC4EAFULL,
        0x6974E718D7D7625BULL, 0x69AA20DF0DCD3AF1ULL, 0x69E0548B68A044D7ULL, 0x6A1469AE42C8560DULL,
        0x6A498419D37A6B90ULL, 0x6A7FE52048590673ULL, 0x6AB3EF342D37A408ULL, 0x6AE8EB0138858D0AULL,
        0x6B1F25C186A6F04DULL, 0x6B537798F4285630ULL, 0x6B88557F31326BBCULL, 0x6BBE6ADEFD7F06ABULL,
        0x6BF302CB5E6F642BULL, 0x6C27C37E360B3D36ULL, 0x6C5DB45DC38E0C83ULL, 0x6C9290BA9A38C7D2ULL,
        0x6CC734E940C6F9C6ULL, 0x6CFD022390F8B838ULL, 0x6D3221563A9B7323ULL, 0x6D66A9ABC9424FECULL,
        0x6D9C5416BB92E3E7ULL, 0x6DD1B48E353BCE70ULL, 0x6E0621B1C28AC20CULL, 0x6E3BAA1E332D728FULL,
        0x6E714A52DFFC679AULL, 0x6EA59CE797FB8180ULL, 0x6EDB04217DFA61E0ULL, 0x6F10E294EEBC7D2CULL,
        0x6F451B3A2A6B9C77ULL, 0x6F7A6208B5068395ULL, 0x6FB07D457124123DULL, 0x6FE49C96CD6D16CCULL,
        0x7019C3BC80C85C7FULL, 0x70501A55D07D39D0ULL, 0x708420EB449C8843ULL, 0x70B9292615C3AA54ULL,
        0x70EF736F9B3494E9ULL, 0x7123A825C100DD12ULL, 0x7158922F31411456ULL, 0x718EB6BAFD91596CULL,
        0x71C33234DE7AD7E3ULL, 0x71F7FEC216198DDCULL, 0x722DFE729B9FF153ULL, 0x7262BF07A143F6D4ULL,
        0x72976EC98994F489ULL, 0x72CD4A7BEBFA31ABULL, 0x73024E8D737C5F0BULL, 0x7336E230D05B76CEULL,
        0x736C9ABD04725481ULL, 0x73A1E0B622C774D1ULL, 0x73D658E3AB795205ULL, 0x740BEF1C9657A686ULL,
        0x74417571DDF6C814ULL, 0x7475D2CE55747A19ULL, 0x74AB4781EAD1989FULL, 0x74E10CB132C2FF64ULL,
        0x75154FDD7F73BF3CULL, 0x754AA3D4DF50AF0BULL, 0x7580A6650B926D67ULL, 0x75B4CFFE4E7708C1ULL,
        0x75EA03FDE214CAF1ULL, 0x7620427EAD4CFED7ULL, 0x7654531E58A03E8CULL, 0x768967E5EEC84E2FULL,
        0x76BFC1DF6A7A61BBULL, 0x76F3D92BA28C7D15ULL, 0x7728CF768B2F9C5AULL, 0x775F03542DFB8371ULL,
        0x779362149CBD3227ULL, 0x77C83A99C3EC7EB0ULL, 0x77FE494034E79E5CULL, 0x7832EDC82110C2FAULL,
        0x7867A93A2954F3B8ULL, 0x789D9388B3AA30A6ULL, 0x78D27C35704A5E68ULL, 0x79071B42CC5CF602ULL,
        0x793CE2137F743382ULL, 0x79720D4C2FA8A031ULL, 0x79A6909F3B92C83EULL, 0x79DC34C70A777A4DULL,
        0x7A11A0FC668AAC70ULL, 0x7A46093B802D578CULL, 0x7A7B8B8A6038AD6FULL, 0x7AB137367C236C66ULL,
        0x7AE585041B2C477FULL, 0x7B1AE64521F7595FULL, 0x7B50CFEB353A97DBULL, 0x7B8503E602893DD2ULL,
        0x7BBA44DF832B8D46ULL, 0x7BF06B0BB1FB384CULL, 0x7C2485CE9E7A065FULL, 0x7C59A742461887F7ULL,
        0x7C9008896BCF54FAULL, 0x7CC40AABC6C32A39ULL, 0x7CF90D56B873F4C7ULL, 0x7D2F50AC6690F1F9ULL,
        0x7D63926BC01A973CULL, 0x7D987706B0213D0AULL, 0x7DCE94C85C298C4DULL, 0x7E031CFD3999F7B0ULL,
        0x7E37E43C8800759CULL, 0x7E6DDD4BAA009303ULL, 0x7EA2AA4F4A405BE2ULL, 0x7ED754E31CD072DAULL,
        0x7F0D2A1BE4048F91ULL, 0x7F423A516E82D9BBULL, 0x7F76C8E5CA239029ULL, 0x7FAC7B1F3CAC7434ULL,
        0x7FE1CCF385EBC8A0ULL,
    };
    return tab[k - kTextPow10Min];
}
// The bits of the smallest double >= (10^16 - 5) * 10^(k - 15), k = 15 .. 308 (index k - 15): a
// value of k + 1 digits at or above it has the image 9.99999999999999|5.. which rounds (ties to
// even: ...999 is odd) to 10^15, one digit more.  Entries past DBL_MAX hold the bits of +Inf,
// which no finite value reaches.  Generated and checked like the table above.
LPR_TEXT_HD uint64_t text_carry_ceil(int k) {
    static constexpr uint64_t tab[kTextPow10Max - 15 + 1] = {
        0x4341C37937E07FFEULL, 0x4376345785D89FFDULL, 0x43ABC16D674EC7FDULL, 0x43E158E460913CFEULL,
        0x4415AF1D78B58C3DULL, 0x444B1AE4D6E2EF4DULL, 0x4480F0CF064DD590ULL, 0x44B52D02C7E14AF4ULL,
        0x44EA784379D99DB1ULL, 0x45208B2A2C28028FULL, 0x4554ADF4B7320332ULL, 0x4589D971E4FE83FFULL,
        0x45C027E72F1F127FULL, 0x45F431E0FAE6D71FULL, 0x46293E5939A08CE7ULL, 0x465F8DEF8808B020ULL,
        0x4693B8B5B5056E14ULL, 0x46C8A6E32246C999ULL, 0x46FED09BEAD87C00ULL, 0x4733426172C74D80ULL,
        0x476812F9CF7920E0ULL, 0x479E17B843576918ULL, 0x47D2CED32A16A1AFULL, 0x48078287F49C4A1BULL,
        0x483D6329F1C35CA1ULL, 0x48725DFA371A19E5ULL, 0x48A6F578C4E0A05EULL, 0x48DCB2D6F618C875ULL,
        0x4911EFC659CF7D4AULL, 0x49466BB7F0435C9CULL, 0x497C06A5EC5433C3ULL, 0x49B18427B3B4A05AULL,
        0x49E5E531A0A1C870ULL, 0x4A1B5E7E08CA3A8CULL, 0x4A511B0EC57E6498ULL, 0x4A8561D276DDFDBEULL,
        0x4ABABA4714957D2DULL, 0x4AF0B46C6CDD6E3CULL, 0x4B24E1878814C9CBULL, 0x4B5A19E96A19FC3EULL,
        0x4B905031E2503DA7ULL, 0x4BC4643E5AE44D10ULL, 0x4BF97D4DF19D6054ULL, 0x4C2FDCA16E04B869ULL,
        0x4C63E9E4E4C2F342ULL, 0x4C98E45E1DF3B012ULL, 0x4CCF1D75A5709C17ULL, 0x4D0372698766618EULL,
        0x4D384F03E93FF9F2ULL, 0x4D6E62C4E38FF86EULL, 0x4DA2FDBB0E39FB45ULL, 0x4DD7BD29D1C87A16ULL,
        0x4E0DAC74463A989CULL, 0x4E428BC8ABE49F62ULL, 0x4E772EBAD6DDC73AULL, 0x4EACFA698C953908ULL,
        0x4EE21C81F7DD43A5ULL, 0x4F16A3A275D4948EULL, 0x4F4C4C8B1349B9B2ULL, 0x4F81AFD6EC0E140FULL,
        0x4FB61BCCA7119913ULL, 0x4FEBA2BFD0D5FF58ULL, 0x502145B7E285BF97ULL, 0x50559725DB272F7DULL,
        0x508AFCEF51F0FB5CULL, 0x50C0DE1593369D19ULL, 0x50F5159AF8044460ULL, 0x512A5B01B6055578ULL,
        0x516078E111C3556BULL, 0x5194971956342AC6ULL, 0x51C9BCDFABC13577ULL, 0x5200160BCB58C16AULL,
        0x52341B8EBE2EF1C5ULL, 0x526922726DBAAE36ULL, 0x529F6B0F092959C3ULL, 0x52D3A2E965B9D81AULL,
        0x53088BA3BF284E21ULL, 0x533EAE8CAEF261A9ULL, 0x53732D17ED577D0AULL, 0x53A7F85DE8AD5C4CULL,
        0x53DDF67562D8B35FULL, 0x5412BA095DC7701BULL, 0x5447688BB5394C22ULL, 0x547D42AEA2879F2BULL,
        0x54B249AD2594C37BULL, 0x54E6DC186EF9F459ULL, 0x551C931E8AB87170ULL, 0x5551DBF316B346E6ULL,
        0x558652EFDC60189FULL, 0x55BBE7ABD3781EC7ULL, 0x55F170CB642B133DULL, 0x5625CCFE3D35D80CULL,
        0x565B403DCC834E0EULL, 0x569108269FD210C9ULL, 0x56C54A3047C694FBULL, 0x56FA9CBC59B83A3AULL,
        0x5730A1F5B8132464ULL, 0x5764CA732617ED7DULL, 0x5799FD0FEF9DE8DDULL, 0x57D03E29F5C2B18AULL,
        0x58044DB473335DEDULL, 0x5839612190003568ULL, 0x586FB969F40042C1ULL, 0x58A3D3E2388029B9ULL,
        0x58D8C8DAC6A03427ULL, 0x590EFB1178484131ULL, 0x59435CEAEB2D28BFULL, 0x59783425A5F872EEULL,
        0x59AE412F0F768FAAULL, 0x59E2E8BD69AA19CAULL, 0x5A17A2ECC414A03DULL, 0x5A4D8BA7F519C84CULL,
        0x5A827748F9301D30ULL, 0x5AB7151B377C247BULL, 0x5AECDA62055B2D9AULL, 0x5B22087D4358FC80ULL,
        0x5B568A9C942F3BA0ULL, 0x5B8C2D43B93B0A88ULL, 0x5BC19C4A53C4E695ULL, 0x5BF6035CE8B6203BULL,
        0x5C2B843422E3A849ULL, 0x5C6132A095CE492EULL, 0x5C957F48BB41DB79ULL, 0x5CCADF1AEA125257ULL,
        0x5D00CB70D24B7377ULL, 0x5D34FE4D06DE5054ULL, 0x5D6A3DE04895E469ULL, 0x5DA066AC2D5DAEC2ULL,
        0x5DD4805738B51A72ULL, 0x5E09A06D06E2610FULL, 0x5E400444244D7CAAULL, 0x5E7405552D60DBD4ULL,
        0x5EA906AA78B912C9ULL, 0x5EDF485516E7577BULL, 0x5F138D352E5096ADULL, 0x5F48708279E4BC58ULL,
        0x5F7E8CA3185DEB6EULL, 0x5FB317E5EF3AB325ULL, 0x5FE7DDDF6B095FEEULL, 0x601DD55745CBB7E9ULL,
        0x6052A5568B9F52F2ULL, 0x60874EAC2E8727AEULL, 0x60BD22573A28F19AULL, 0x60F2357684599700ULL,
        0x6126C2D4256FFCC0ULL, 0x615C73892ECBFBF0ULL, 0x6191C835BD3F7D76ULL, 0x61C63A432C8F5CD4ULL,
        0x61FBC8D3F7B33409ULL, 0x62315D847AD00086ULL, 0x6265B4E5998400A7ULL, 0x629B221EFFE500D0ULL,
        0x62D0F5535FEF2082ULL, 0x630532A837EAE8A3ULL, 0x633A7F5245E5A2CCULL, 0x63708F936BAF85BFULL,
        0x63A4B378469B672FULL, 0x63D9E056584240FBULL, 0x64102C35F729689DULL, 0x6444374374F3C2C4ULL,
        0x647945145230B375ULL, 0x64AF965966BCE052ULL, 0x64E3BDF7E0360C33ULL, 0x6518AD75D8438F40ULL,
        0x654ED8D34E547310ULL, 0x6583478410F4C7EAULL, 0x65B819651531F9E5ULL, 0x65EE1FBE5A7E785EULL,
        0x6622D3D6F88F0B3BULL, 0x665788CCB6B2CE09ULL, 0x668D6AFFE45F818CULL, 0x66C262DFEEBBB0F7ULL,
        0x66F6FB97EA6A9D35ULL, 0x672CBA7DE5054482ULL, 0x6761F48EAF234AD2ULL, 0x679671B25AEC1D86ULL,
        0x67CC0E1EF1A724E7ULL, 0x680188D357087711ULL, 0x6835EB082CCA94D5ULL, 0x686B65CA37FD3A0AULL,
        0x68A11F9E62FE4446ULL, 0x68D56785FBBDD558ULL, 0x690AC1677AAD4AAEULL, 0x6940B8E0ACAC4EADULL,
        0x6974E718D7D76258ULL, 0x69AA20DF0DCD3AEEULL, 0x69E0548B68A044D5ULL, 0x6A1469AE42C8560AULL,
        0x6A498419D37A6B8CULL, 0x6A7FE5204859066FULL, 0x6AB3EF342D37A405ULL, 0x6AE8EB0138858D07ULL,
        0x6B1F25C186A6F048ULL, 0x6B537798F428562DULL, 0x6B88557F31326BB9ULL, 0x6BBE6ADEFD7F06A7ULL,
        0x6BF302CB5E6F6428ULL, 0x6C27C37E360B3D32ULL, 0x6C5DB45DC38E0C7FULL, 0x6C9290BA9A38C7CFULL,
        0x6CC734E940C6F9C3ULL, 0x6CFD022390F8B834ULL, 0x6D3221563A9B7321ULL, 0x6D66A9ABC9424FE9ULL,
        0x6D9C5416BB92E3E3ULL, 0x6DD1B48E353BCE6EULL, 0x6E0621B1C28AC209ULL, 0x6E3BAA1E332D728BULL,
        0x6E714A52DFFC6797ULL, 0x6EA59CE797FB817DULL, 0x6EDB04217DFA61DCULL, 0x6F10E294EEBC7D2AULL,
        0x6F451B3A2A6B9C74ULL, 0x6F7A6208B5068391ULL, 0x6FB07D457124123BULL, 0x6FE49C96CD6D16C9ULL,
        0x7019C3BC80C85C7BULL, 0x70501A55D07D39CDULL, 0x708420EB449C8841ULL, 0x70B9292615C3AA51ULL,
        0x70EF736F9B3494E5ULL, 0x7123A825C100DD0FULL, 0x7158922F31411453ULL, 0x718EB6BAFD915967ULL,
        0x71C33234DE7AD7E1ULL, 0x71F7FEC216198DD9ULL, 0x722DFE729B9FF14FULL, 0x7262BF07A143F6D1ULL,
        0x72976EC98994F486ULL, 0x72CD4A7BEBFA31A7ULL, 0x73024E8D737C5F09ULL, 0x7336E230D05B76CBULL,
        0x736C9ABD0472547DULL, 0x73A1E0B622C774CEULL, 0x73D658E3AB795202ULL, 0x740BEF1C9657A682ULL,
        0x74417571DDF6C812ULL, 0x7475D2CE55747A16ULL, 0x74AB4781EAD1989BULL, 0x74E10CB132C2FF61ULL,
        0x75154FDD7F73BF39ULL, 0x754AA3D4DF50AF08ULL, 0x7580A6650B926D65ULL, 0x75B4CFFE4E7708BEULL,
        0x75EA03FDE214CAEDULL, 0x7620427EAD4CFED5ULL, 0x7654531E58A03E8AULL, 0x768967E5EEC84E2CULL,
        0x76BFC1DF6A7A61B7ULL, 0x76F3D92BA28C7D12ULL, 0x7728CF768B2F9C57ULL, 0x775F03542DFB836CULL,
        0x779362149CBD3224ULL, 0x77C83A99C3EC7EADULL, 0x77FE494034E79E58ULL, 0x7832EDC82110C2F7ULL,
        0x7867A93A2954F3B5ULL, 0x789D9388B3AA30A2ULL, 0x78D27C35704A5E65ULL, 0x79071B42CC5CF5FFULL,
        0x793CE2137F74337EULL, 0x79720D4C2FA8A02FULL, 0x79A6909F3B92C83BULL, 0x79DC34C70A777A49ULL,
        0x7A11A0FC668AAC6EULL, 0x7A46093B802D5789ULL, 0x7A7B8B8A6038AD6BULL, 0x7AB137367C236C63ULL,
        0x7AE585041B2C477CULL, 0x7B1AE64521F7595BULL, 0x7B50CFEB353A97D9ULL, 0x7B8503E602893DCFULL,
        0x7BBA44DF832B8D43ULL, 0x7BF06B0BB1FB384AULL, 0x7C2485CE9E7A065CULL, 0x7C59A742461887F3ULL,
        0x7C9008896BCF54F8ULL, 0x7CC40AABC6C32A36ULL, 0x7CF90D56B873F4C4ULL, 0x7D2F50AC6690F1F4ULL,
        0x7D63926BC01A9739ULL, 0x7D987706B0213D07ULL, 0x7DCE94C85C298C49ULL, 0x7E031CFD3999F7AEULL,
        0x7E37E43C88007599ULL, 0x7E6DDD4BAA0092FFULL, 0x7EA2AA4F4A405BDFULL, 0x7ED754E31CD072D7ULL,
        0x7F0D2A1BE4048F8DULL, 0x7F423A516E82D9B8ULL, 0x7F76C8E5CA239026ULL, 0x7FAC7B1F3CAC7430ULL,
        0x7FE1CCF385EBC89EULL, 0x7FF0000000000000ULL,
    };
    return tab[k - 15];
}

// k with 10^k <= |v| < 10^(k+1) for a normal |v| >= 1e-4 (bits a).  floor(E * log10(2)) is k or
// k - 1 for E = floor(log2 |v|); 315653 / 2^20 is log10(2) less 2.6e-8, at most 2.7e-5 over the
// range, and no E in -14 .. 1023 has E * log10(2) closer than 1.4e-3 above an integer, so the
// shift gives that floor (checked against exact powers for every E); one exact comparison
// settles the rest.
LPR_TEXT_HD int text_decade(uint64_t a) {
    const int E = (int)(a >> 52) - 1023;
    int k = (E * 315653) >> 20;
    if (k < kTextPow10Max && a >= text_pow10_ceil(k + 1)) ++k;
    return k;
}

LPR_TEXT_HD int text_ndigits32(uint32_t v) {
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) +
           (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
LPR_TEXT_HD int text_ndigits64(uint64_t v) {  // v < 10^17
    const uint32_t hi = (uint32_t)(v / 100000000ull);
    return hi ? 8 + text_ndigits32(hi) : text_ndigits32((uint32_t)v);
}

// (n + d / 2) / d for d = 10^p, p = 1 .. 18, every divisor a constant (a multiply and a shift on
// the device, no division routine).
LPR_TEXT_HD uint64_t text_div_pow10_half_up(uint64_t n, int p) {
#define LPR_TEXT_CASE(P) \
    case P:              \
        return (n + text_ipow(10, P) / 2) / text_ipow(10, P);
    switch (p) {
        LPR_TEXT_CASE(1) LPR_TEXT_CASE(2) LPR_TEXT_CASE(3) LPR_TEXT_CASE(4) LPR_TEXT_CASE(5)
        LPR_TEXT_CASE(6) LPR_TEXT_CASE(7) LPR_TEXT_CASE(8) LPR_TEXT_CASE(9) LPR_TEXT_CASE(10)
        LPR_TEXT_CASE(11) LPR_TEXT_CASE(12) LPR_TEXT_CASE(13) LPR_TEXT_CASE(14) LPR_TEXT_CASE(15)
        LPR_TEXT_CASE(16) LPR_TEXT_CASE(17) LPR_TEXT_CASE(18)
    }
#undef LPR_TEXT_CASE
    return n;
}

// Thousandths T of kTextF3Threshold <= |v| < 1e15 (bits a): |v| = m * 2^e, s = 14 - k,
// N = round-half-even(m * 5^s * 2^(e + s)) is the 15-digit image as an integer (10^14 <= N <=
// 10^15), T = N * 10^(3 - s) or round-half-up(N / 10^(s - 3)).  e + s < 0 throughout the range
// (N < 2^50 while m * 5^s >= 2^52), so the scaling is a right shift with an exact remainder; the
// widest intermediate, m * 5^18, has 95 bits.
LPR_TEXT_HD uint64_t text_fast_thousandths(uint64_t a) {
    static constexpr uint64_t p5[19] = {
        text_ipow(5, 0),  text_ipow(5, 1),  text_ipow(5, 2),  text_ipow(5, 3),  text_ipow(5, 4),
        text_ipow(5, 5),  text_ipow(5, 6),  text_ipow(5, 7),  text_ipow(5, 8),  text_ipow(5, 9),
        text_ipow(5, 10), text_ipow(5, 11), text_ipow(5, 12), text_ipow(5, 13), text_ipow(5, 14),
        text_ipow(5, 15), text_ipow(5, 16), text_ipow(5, 17), text_ipow(5, 18)};
    const uint64_t m = (a & ((1ull << 52) - 1)) | (1ull << 52);
    const int e = (int)(a >> 52) - 1075;
    const int s = 14 - text_decade(a);  // 0 .. 18
    const unsigned __int128 P = (unsigned __int128)m * p5[s];
    const int sh = -(e + s);  // 1 .. 50
    uint64_t N = (uint64_t)(P >> sh);
    const unsigned __int128 half = (unsigned __int128)1 << (sh - 1);
    const unsigned __int128 rem = P & ((half << 1) - 1);
    if (rem > half || (rem == half && (N & 1))) ++N;
    static_assert(kTextDecimals == 3, "the multipliers below are 10^(3 - s)");
    if (s <= kTextDecimals) return N * (s == 0 ? 1000u : s == 1 ? 100u : s == 2 ? 10u : 1u);
    return text_div_pow10_half_up(N, s - kTextDecimals);
}

// One measured cell: what the write pass needs to put its bytes without converting again.
struct TextCell {
    uint64_t T;   // fast: thousandths; big: the bits of |v|
    int32_t len;  // bytes of the cell
    uint8_t cls;  // TextClass
    uint8_t neg;  // a "-" is printed
};

// Digits of |v| >= 1e15 before the point: k + 1, and one more when the image carries to 10^15.
LPR_TEXT_HD int text_big_digits(uint64_t a) {
    const int k = text_decade(a);
    return k + 1 + (a >= text_carry_ceil(k) ? 1 : 0);
}

LPR_TEXT_HD TextCell text_cell_measure(uint64_t bits) {
    const uint64_t a = bits & kTextAbsMask;
    const bool neg = (bits >> 63) != 0;
    TextCell c;
    c.T = 0;
    c.neg = 0;
    if (a > kTextInfBits) {
        c.cls = kTextNaN;
        c.len = 3;
    } else if (a == kTextInfBits) {
        c.cls = neg ? kTextNegInf : kTextPosInf;
        c.len = neg ? 9 : 8;
    } else if (a < kTextF3Threshold) {
        c.cls = kTextZero;
        c.len = 2 + kTextDecimals;
    } else if (a < kTextBigBits) {
        c.cls = kTextFast;
        c.T = text_fast_thousandths(a);
        c.neg = neg;
        c.len = (int32_t)neg + text_ndigits64(c.T / 1000u) + 1 + kTextDecimals;
    } else {
        c.cls = kTextBig;
        c.T = a;
        c.neg = neg;
        c.len = (int32_t)neg + text_big_digits(a) + 1 + kTextDecimals;
    }
    return c;
}

LPR_TEXT_HD void text_put_literal(uint8_t* dst, const char* s, int n) {
    for (int i = 0; i < n; ++i) dst[i] = (uint8_t)s[i];
}
// v in nd decimal digits at dst (leading zeros when v has fewer)
LPR_TEXT_HD void text_put_uint32(uint8_t* dst, uint32_t v, int nd) {
    for (int i = nd - 1; i >= 0; --i) {
        const uint32_t q = v / 10u;
        dst[i] = (uint8_t)('0' + (v - q * 10u));
        v = q;
    }
}
LPR_TEXT_HD void text_put_uint64(uint8_t* dst, uint64_t v, int nd) {  // v < 10^16
    const uint32_t hi = (uint32_t)(v / 100000000ull), lo = (uint32_t)(v - hi * 100000000ull);
    if (nd > 8) {
        text_put_uint32(dst, hi, nd - 8);
        text_put_uint32(dst + nd - 8, lo, 8);
    } else {
        text_put_uint32(dst, lo, nd);
    }
}

// The bytes of every cell but a big one (those go through text_big_put); c.len bytes at dst.
LPR_TEXT_HD void text_cell_put(const TextCell& c, uint8_t* dst) {
    switch (c.cls) {
    case kTextNaN: text_put_literal(dst, "NaN", 3); break;
    case kTextPosInf: text_put_literal(dst, "Infinity", 8); break;
    case kTextNegInf: text_put_literal(dst, "-Infinity", 9); break;
    case kTextZero: text_put_literal(dst, "0.000", 5); break;
    case kTextFast: {
        const uint64_t ip = c.T / 1000u;
        const uint32_t fp = (uint32_t)(c.T - ip * 1000u);
        const int nd = c.len - (int)c.neg - 1 - kTextDecimals;
        if (c.neg) dst[0] = '-';
        text_put_uint64(dst + c.neg, ip, nd);
        dst[c.neg + nd] = '.';
        text_put_uint32(dst + c.neg + nd + 1, fp, kTextDecimals);
        break;
    }
    default: break;
    }
}

// The slow path, |v| >= 1e15 (bits a): the integer m * 2^e of up to 1024 bits (e >= -3: the low
// bits of a value just above 1e15 are a binary fraction and only make the remainder sticky) in
// 32-bit words, divided by 10^9 until nothing is left -- at most 35 chunks of nine digits -- then
// walked from the top: 15 digits into *Q, the 16th and whether anything non-zero follows decide
// the rounding, exact ties to even.  *Q can be 10^15.  *D: digits of the integer part.
LPR_TEXT_HD void text_big_image(uint64_t a, uint64_t* Q, int* D) {
    uint32_t w[33], c[35];
    uint64_t m = (a & ((1ull << 52) - 1)) | (1ull << 52);
    int e = (int)(a >> 52) - 1075;
    bool sticky = false;
    if (e < 0) {
        sticky = (m & ((1ull << -e) - 1)) != 0;
        m >>= -e;
        e = 0;
    }
    for (int i = 0; i < 33; ++i) w[i] = 0;
    const int wi = e >> 5, b = e & 31;  // wi <= 30
    const uint64_t lo = (m & 0xffffffffull) << b, hi = ((m >> 32) << b) + (lo >> 32);
    w[wi] = (uint32_t)lo;
    w[wi + 1] = (uint32_t)hi;
    w[wi + 2] = (uint32_t)(hi >> 32);
    int n = wi + 3, nc = 0;
    while (n > 0 && w[n - 1] == 0) --n;
    while (n > 0) {
        uint64_t r = 0;
        for (int i = n - 1; i >= 0; --i) {
            const uint64_t cur = (r << 32) | w[i];
            const uint64_t q = cur / 1000000000ull;
            w[i] = (uint32_t)q;
            r = cur - q * 1000000000ull;
        }
        c[nc++] = (uint32_t)r;
        while (n > 0 && w[n - 1] == 0) --n;
    }
    const int top = text_ndigits32(c[nc - 1]);
    *D = 9 * (nc - 1) + top;
    uint64_t q = 0;
    int cnt = 0;
    uint32_t d16 = 0;
    for (int ci = nc - 1; ci >= 0; --ci) {
        uint32_t v = c[ci];
        if (cnt > 15) {
            sticky = sticky || v != 0;
            continue;
        }
        uint32_t p = (uint32_t)text_ipow(10, 8);
        int nd = 9;
        if (ci == nc - 1)
            for (; nd > top; --nd) p /= 10u;
        for (int d = 0; d < nd; ++d, p /= 10u) {
            const uint32_t digit = v / p;
            v -= digit * p;
            if (cnt < 15)
                q = q * 10u + digit;
            else if (cnt == 15)
                d16 = digit;
            else
                sticky = sticky || digit != 0;
            ++cnt;
        }
    }
    if (d16 > 5 || (d16 == 5 && (sticky || (q & 1)))) ++q;
    *Q = q;
}

// The bytes of a big cell: sign, the image, zeros up to the point, ".000".  Returns their count,
// which is TextCell::len of the same value (text_big_digits states the same digits from two
// comparisons; tools/text_format_check.cpp holds the two against each other).
LPR_TEXT_HD int text_big_put(uint64_t bits, uint8_t* dst) {
    const uint64_t a = bits & kTextAbsMask;
    uint64_t Q;
    int D;
    text_big_image(a, &Q, &D);
    int at = 0;
    if (bits >> 63) dst[at++] = '-';
    const int nq = Q >= text_ipow(10, 15) ? 16 : 15;
    text_put_uint64(dst + at, Q, nq);
    at += nq;
    for (int i = 15; i < D; ++i) dst[at++] = '0';
    dst[at++] = '.';
    for (int i = 0; i < kTextDecimals; ++i) dst[at++] = '0';
    return at;
}

// ---------------------------------------------------------------- the block layout (:22-48)
//   "-" x 80 CRLF
//   "Table\t" "x1\t" .. "x{nvars}\t" "t1\t" .. "t{cols - 1 - nvars}\t" "RHS" CRLF
//   "Z\t" cell "\t" .. cell "\t" CRLF, then "{i}\t" .. for i = 1 .. rows - 1
constexpr int kTextDashes = 80;
constexpr int64_t kTextRuleLen = kTextDashes + 2;  // the dashes and their CRLF
constexpr int64_t kTextTableLen = 6;               // "Table\t"

// sum of the decimal digits counts of 1 .. n
LPR_TEXT_HD int64_t text_sum_ndigits(int64_t n) {
    int64_t s = 0;
    for (int64_t p = 1; p <= n; p *= 10) s += n - p + 1;
    return s;
}
// bytes of "x1\t" .. "x{n}\t" (or t): a letter, the digits and a tab each
LPR_TEXT_HD int64_t text_labels_len(int64_t n) { return n <= 0 ? 0 : 2 * n + text_sum_ndigits(n); }
LPR_TEXT_HD int64_t text_tcount(int32_t cols, int32_t nvars) {
    return (int64_t)cols - 1 - nvars > 0 ? (int64_t)cols - 1 - nvars : 0;
}
// the rule and the "Table" line
LPR_TEXT_HD int64_t text_header_len(int32_t cols, int32_t nvars) {
    return kTextRuleLen + kTextTableLen + text_labels_len(nvars) +
           text_labels_len(text_tcount(cols, nvars)) + 5;
}
static_assert(kTextRuleLen == 82 && kTextTableLen == 6, "\"-\" x 80 CRLF, \"Table\\t\"");
// "Z" or the decimal row index, without the tab
LPR_TEXT_HD int text_row_label_len(int32_t i) { return i == 0 ? 1 : text_ndigits32((uint32_t)i); }
// bytes of a row besides its cells' own: label, its tab, one tab per cell, CRLF
LPR_TEXT_HD int64_t text_row_frame_len(int32_t i, int32_t cols) {
    return text_row_label_len(i) + 1 + (int64_t)cols + 2;
}

// One block of a call, in device memory.  A row is converted by `lanes` adjacent lanes of a wave
// (a power of two, 4 .. 64, the smallest that holds cols), so a wave takes 64 / lanes rows of one
// block at a time: a wave task.  round4 is how many times Math.Round(v, 4) is applied to a cell
// before it is formatted (0, 1 or 2: DisplayTableau); only the rounded
// kernels read it.  The host owns every field.
struct TextBlock {
    const double* src;  // rows x cols row-major, where the source keeps it
    int64_t row0;       // the block's first row among all rows of the call
    int64_t wave0;      // its first wave task among all of the call
    int64_t hdr_end;    // bytes of the rule and "Table" lines of blocks 0 .. this one
    int32_t rows, cols, nvars;
    int16_t lanes, round4;
};
static_assert(sizeof(TextBlock) == 48, "TextBlock is 48 bytes: round4 took half of lanes' word");
constexpr int kTextMaxRound4 = 2;
constexpr int text_lanes(int32_t cols) {
    int l = 4;
    while (l < 64 && l < cols) l *= 2;
    return l;
}
static_assert(text_lanes(1) == 4 && text_lanes(5) == 8 && text_lanes(64) == 64 &&
              text_lanes(65) == 64, "the smallest power of two in 4 .. 64 that holds cols");
// A cell of 1e15 or more, listed by the write pass for the slow-path kernel: its bits and where
// its bytes start in the text.
struct TextBigCell {
    uint64_t bits;
    int64_t at;
};
constexpr int kTextScanTile = 2048;  // rows one workgroup scans: 256 lanes x 8

}  // namespace lpr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <vector>
struct lpr_engine;
struct lpr_text;
namespace lpr {
// text_engine.hip: blocks whose src (device memory that stays as it is until the call returns),
// rows, cols, nvars and round4 are set -> an lpr_text on e; what lpr_bb_batch_narrate_text
// (bb_batch_engine.hip) ends in.  W names the call in error messages.
int text_format_blocks(const char* W, lpr_engine* e, std::vector<TextBlock>& blk, lpr_text** out);
// text_kernels.hip: the launchers text_engine.hip calls, all on stream s.  rows_scan is
// row_len[n_rows + 1] (the last entry 0): row lengths after text_launch_measure, their exclusive
// prefix (the last entry the total) after text_launch_scan; partials holds
// ceil((n_rows + 1) / kTextScanTile) entries.  `rounded` picks the instantiation of the two passes
// that applies TextBlock::round4 (the same for both); false where every block has round4 == 0.
void text_launch_measure(hipStream_t s, bool rounded, const TextBlock* blk, int64_t n_blk,
                         int64_t n_tasks, int64_t* rows_scan, uint32_t* big_count);
void text_launch_scan(hipStream_t s, int64_t* rows_scan, int64_t n, int64_t* partials);
void text_launch_offsets(hipStream_t s, const TextBlock* blk, int64_t n_blk, int64_t n_rows,
                         const int64_t* rows_scan, int64_t* offsets);
void text_launch_write(hipStream_t s, bool rounded, const TextBlock* blk, int64_t n_blk,
                       int64_t n_tasks, const int64_t* rows_scan, uint8_t* text, TextBigCell* big,
                       uint32_t big_cap, uint32_t* big_fill);
void text_launch_big(hipStream_t s, const TextBigCell* big, uint32_t n, uint8_t* text);
}  // namespace lpr
#endif
